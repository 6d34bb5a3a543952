"""Gemma-2 goldens (tests/golden/gemma2_tiny_*.npz): runs the reference's Gemma2ForCausalLMPatched (model/llm.py:457-567,
eager attention) in fp32 and bf16 on tiny configs whose weights synth_gemma2_state rebuilds from a seed, and stores data
only -- the keys of gemma_tiny_*.npz. Run on a CPU machine with the reference tree:
    python -m tests.gen_goldens_gemma2 <reference dir> [out dir]
The archives are written with fixed zip timestamps (save_npz_fixed), so a rerun reproduces them byte for byte.

With 0.02-wide weights a tiny model's attention scores and logits are about 0.1 and a cap of 50 or 30 would be invisible, so
each config picks its weight width and caps such that BOTH caps matter: the generator reruns the fp32 model with either cap
set to None and refuses to write a file unless each rerun moves logits_fp32 by at least ten times the tolerance the GPU test
holds the prefill to (golden_tolerance below, computed from the archive's own two precisions)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from llamarec_amd.synth import synth_gemma2_state
from tests.gen_goldens_gemma import save_npz_fixed

GEMMA2_CONFIGS = {
    # name: (vocab, hidden, inter, layers, heads, kv_heads, head_dim, query_pre_attn_scalar, attn cap, final cap, weight width)
    "tiny_hd256_gqa": (320, 256, 512, 2, 4, 2, 256, 256, 1.0, 8.0, 0.1),    # gemma-2-2b / 9b: GQA, scalar = head_dim
    "tiny_hd256_qpas": (320, 256, 512, 2, 2, 1, 256, 144, 1.0, 8.0, 0.1),   # gemma-2-27b's scalar 144 != head_dim
    "tiny_hd16": (320, 64, 128, 2, 4, 2, 16, 16, 1.0, 4.0, 0.2),            # the generic attention kernel
}
LABEL_IDS = list(range(40, 60))
LENS = [37, 5, 64, 1, 20, 130]
PREFILL_TOL = 3e-2      # Gemma v1's bound on the prefill against its goldens


def golden_tolerance(logits_fp32, logits_bf16):
    """The GPU test's bound for an archive: Gemma v1's 3e-2 while the reference's own two precisions agree to a third of it,
    otherwise three times their distance."""
    gap = float(np.abs(np.asarray(logits_bf16) - np.asarray(logits_fp32)).max())
    return PREFILL_TOL if gap <= PREFILL_TOL / 3 else 3.0 * gap


def gemma2_cfg_dict(name):
    v, d, f, nl, nh, nkv, hd, qpas, acap, fcap, _ = GEMMA2_CONFIGS[name]
    return dict(model_type="gemma2", vocab_size=v, hidden_size=d, intermediate_size=f, num_hidden_layers=nl,
                num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd, max_position_embeddings=256,
                rms_norm_eps=1e-6, rope_theta=10000.0, hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=qpas,
                attn_logit_softcapping=acap, final_logit_softcapping=fcap, sliding_window=192)


def hf_model(cd, sd, **override):
    from transformers import Gemma2Config, Gemma2ForCausalLM

    kw = {k: v for k, v in dict(cd, **override).items() if k not in ("model_type", "rope_theta")}
    try:
        cfg = Gemma2Config(**kw, rope_parameters={"rope_type": "default", "rope_theta": cd["rope_theta"]},
                           attention_bias=False, tie_word_embeddings=True, attn_implementation="eager")
    except TypeError:
        cfg = Gemma2Config(**kw, rope_theta=cd["rope_theta"], attention_bias=False, tie_word_embeddings=True,
                           attn_implementation="eager")
    model = Gemma2ForCausalLM(cfg).eval()
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not [k for k in missing.missing_keys if "rotary" not in k and k != "lm_head.weight"], missing
    assert not missing.unexpected_keys, missing
    assert torch.equal(model.lm_head.weight, model.model.embed_tokens.weight)   # tied
    return model


def main(REF, OUT):
    sys.path.insert(0, REF)
    import model.llm as ML  # noqa: F401  (patches Gemma2ForCausalLM.forward at import, model/llm.py:567)

    torch.manual_seed(0)
    for ci, name in enumerate(GEMMA2_CONFIGS):
        cd = gemma2_cfg_dict(name)
        seed = 400 + ci
        sd = synth_gemma2_state(cd, seed, std=GEMMA2_CONFIGS[name][-1])
        model = hf_model(cd, sd)
        rng = np.random.default_rng(seed)
        T = max(LENS)
        assert T < cd["sliding_window"]
        ids = np.zeros((len(LENS), T), np.int64)
        mask = np.zeros((len(LENS), T), np.int64)
        for b, n in enumerate(LENS):
            ids[b, T - n:] = rng.integers(3, cd["vocab_size"], size=n)
            ids[b, T - n] = 2   # <bos> of the Gemma tokenizer
            mask[b, T - n:] = 1
        labels = np.zeros((len(LENS), 1), np.int64)
        tids, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
        with torch.no_grad():
            o32 = model(input_ids=tids, attention_mask=tmask, labels=torch.from_numpy(labels))
            loss = float(o32.loss)
            l32 = o32.logits.numpy()
            lun = np.stack([model(input_ids=tids[b:b + 1, T - n:]).logits[0].numpy() for b, n in enumerate(LENS)])
            moved = {k: float(np.abs(hf_model(cd, sd, **{k: None})(input_ids=tids, attention_mask=tmask).logits.numpy()
                                     - l32).max())
                     for k in ("attn_logit_softcapping", "final_logit_softcapping")}
            mb = model.to(torch.bfloat16)
            lbf = mb(input_ids=tids, attention_mask=tmask).logits
            assert lbf.dtype == torch.float32
            lbf = lbf.numpy()
        assert l32.shape == (len(LENS), cd["vocab_size"]) and loss == -1.0
        tol = golden_tolerance(l32, lbf)
        print(f"{name}: max |logit| {np.abs(l32).max():.3f}, bf16-fp32 {np.abs(lbf - l32).max():.4f}, tolerance {tol:.4f}, "
              f"without the attention cap {moved['attn_logit_softcapping']:.3f}, without the final cap "
              f"{moved['final_logit_softcapping']:.3f}")
        for k, m in moved.items():
            assert m >= 10 * tol, f"{name}: dropping {k} moves logits_fp32 by {m}, less than ten times the tolerance {tol}"
        save_npz_fixed(os.path.join(OUT, f"gemma2_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(seed), weight_std=np.array(GEMMA2_CONFIGS[name][-1]), input_ids=ids,
                       attention_mask=mask, lens=np.array(LENS), logits_fp32=l32, logits_fp32_unpadded=lun, logits_bf16=lbf,
                       eval_loss=np.array(loss), label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS],
                       scores_bf16=lbf[:, LABEL_IDS])


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_gemma2 <reference tree> [out dir]")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out)
