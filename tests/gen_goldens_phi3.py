"""Phi-3 goldens (tests/golden/phi3_tiny_*.npz): runs the reference's Phi3ForCausalLMPatched (model/llm.py:148-248, eager
attention) in fp32 and bf16 on tiny configs whose weights synth_phi3_state rebuilds from a seed, and stores data only -- the
keys of gemma2_tiny_*.npz. Run on a CPU machine with the reference tree:
    python -m tests.gen_goldens_phi3 <reference dir> [out dir]
The archives are written with fixed zip timestamps (save_npz_fixed), so a rerun reproduces them byte for byte.

Before a file is written the generator asserts that the goldens are Phi-3's own: reading gate_up_proj's halves the other way
round, or qkv_proj as stored group by group, must move logits_fp32 by at least ten times the tolerance the GPU test holds the
prefill to (golden_tolerance, computed from the archive's own two precisions). Both misreadings are evaluated with the fp32
restatement tests/phi3_ref.py, which must itself sit on the reference's fp32 logits."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from llamarec_amd.synth import synth_phi3_state
from tests.gen_goldens_gemma import save_npz_fixed
from tests.gen_goldens_gemma2 import golden_tolerance  # noqa: F401  (the GPU test's bound; re-exported)

PHI3_CONFIGS = {
    # name: (vocab, hidden, inter, layers, heads, kv_heads, weight width)
    "hd96_mha": (320, 768, 1024, 2, 8, 8, 0.02),    # Phi-3-mini's head: qkv width 2304 = 9 x 256, heads straddle GEMM tiles
    "hd96_gqa": (320, 384, 512, 2, 4, 2, 0.02),     # GQA at head_dim 96 (Phi-3-medium groups its heads, at 128)
    "hd16": (320, 64, 128, 2, 4, 2, 0.07),          # the generic attention kernel
}
LABEL_IDS = list(range(40, 60))
LENS = [37, 5, 64, 1, 20, 130]


def phi3_cfg_dict(name):
    v, d, f, nl, nh, nkv, _ = PHI3_CONFIGS[name]
    return dict(model_type="phi3", vocab_size=v, hidden_size=d, intermediate_size=f, num_hidden_layers=nl,
                num_attention_heads=nh, num_key_value_heads=nkv, max_position_embeddings=256,
                original_max_position_embeddings=256, rms_norm_eps=1e-5, rope_theta=10000.0, rope_scaling=None,
                hidden_act="silu", sliding_window=192, tie_word_embeddings=False)


def hf_model(cd, sd):
    from transformers import Phi3Config, Phi3ForCausalLM

    kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta", "rope_scaling")}
    kw.update(attention_dropout=0.0, resid_pdrop=0.0, embd_pdrop=0.0, pad_token_id=0, bos_token_id=1, eos_token_id=2,
              attn_implementation="eager")
    try:
        cfg = Phi3Config(**kw, rope_parameters={"rope_type": "default", "rope_theta": cd["rope_theta"]})
    except TypeError:
        cfg = Phi3Config(**kw, rope_theta=cd["rope_theta"], rope_scaling=None)
    model = Phi3ForCausalLM(cfg).eval()
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not [k for k in missing.missing_keys if "rotary" not in k], missing
    assert not missing.unexpected_keys, missing
    assert model.lm_head.weight.data_ptr() != model.model.embed_tokens.weight.data_ptr()   # untied
    return model


def main(REF, OUT):
    sys.path.insert(0, REF)
    import model.llm as ML  # noqa: F401  (patches Phi3ForCausalLM.forward at import, model/llm.py:248)

    from tests import phi3_ref as PR

    torch.manual_seed(0)
    for ci, name in enumerate(PHI3_CONFIGS):
        cd = phi3_cfg_dict(name)
        seed = 500 + ci
        std = PHI3_CONFIGS[name][-1]
        sd = synth_phi3_state(cd, seed, std=std)
        model = hf_model(cd, sd)
        rng = np.random.default_rng(seed)
        T = max(LENS)
        assert T < cd["sliding_window"]
        ids = np.zeros((len(LENS), T), np.int64)
        mask = np.zeros((len(LENS), T), np.int64)
        for b, n in enumerate(LENS):
            ids[b, T - n:] = rng.integers(3, cd["vocab_size"], size=n)
            ids[b, T - n] = 1   # <s>
            mask[b, T - n:] = 1
        labels = np.zeros((len(LENS), 1), np.int64)
        tids, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
        with torch.no_grad():
            o32 = model(input_ids=tids, attention_mask=tmask, labels=torch.from_numpy(labels))
            loss = float(o32.loss)
            l32 = o32.logits.numpy()
            lun = np.stack([model(input_ids=tids[b:b + 1, T - n:]).logits[0].numpy() for b, n in enumerate(LENS)])
            mb = model.to(torch.bfloat16)
            lbf = mb(input_ids=tids, attention_mask=tmask).logits
            assert lbf.dtype == torch.float32
            lbf = lbf.numpy()
        assert l32.shape == (len(LENS), cd["vocab_size"]) and loss == -1.0
        tol = golden_tolerance(l32, lbf)
        seqs = [ids[b, T - n:] for b, n in enumerate(LENS)]
        restated = PR.last_logits(sd, cd, seqs)
        moved = {m: float(np.abs(PR.last_logits(sd, cd, seqs, mutant=m) - l32).max()) for m in ("swap_gate_up", "interleaved_qkv")}
        print(f"{name}: max |logit| {np.abs(l32).max():.3f}, bf16-fp32 {np.abs(lbf - l32).max():.4f}, tolerance {tol:.4f}, "
              f"restatement-fp32 {np.abs(restated - l32).max():.2e}, gate/up swapped {moved['swap_gate_up']:.3f}, "
              f"qkv read group by group {moved['interleaved_qkv']:.3f}")
        assert np.abs(restated - l32).max() < 1e-3 * max(1.0, np.abs(l32).max())
        for m, dist in moved.items():
            assert dist >= 10 * tol, f"{name}: the {m} misreading moves logits_fp32 by {dist}, less than ten times the tolerance {tol}"
        save_npz_fixed(os.path.join(OUT, f"phi3_tiny_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(seed), weight_std=np.array(std), input_ids=ids,
                       attention_mask=mask, lens=np.array(LENS), logits_fp32=l32, logits_fp32_unpadded=lun, logits_bf16=lbf,
                       eval_loss=np.array(loss), label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS],
                       scores_bf16=lbf[:, LABEL_IDS])


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_phi3 <reference tree> [out dir]")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out)
