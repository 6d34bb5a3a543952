"""Qwen3 goldens (tests/golden/qwen3_tiny_*.npz): runs HF Qwen3ForCausalLM (eager attention) in fp32 and bf16 on tiny configs
whose weights synth_qwen3_state rebuilds from a seed, takes the logits at each prompt's last token as the reference's patched
forwards do (model/llm.py: logits[:, -1].float(), eval loss the constant -1), and stores data only -- the keys of
qwen2_tiny_*.npz with qk_norm_spread in place of the two bias widths. The reference has no --llm qwen3; its tree only has to be
present (the generators run where it is), nothing of it is read. Run on a CPU machine:
    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python -m tests.gen_goldens_qwen3 <reference dir> [out dir]
The archives are written with fixed zip timestamps (save_npz_fixed), so a rerun with the same thread count (one: the order of
torch's CPU sums follows it) reproduces them byte for byte.

Before a file is written the generator asserts that the goldens are Qwen3's own: HF's fp32 logits with both norm weights of
every layer replaced by ones must lie more than ten times the tolerance the GPU test holds the prefill to (golden_tolerance,
computed from the archive's own two precisions) from logits_fp32; the fp32 restatement tests/qwen3_ref.py must sit on the
reference's logits and its ones_norm mutant on HF's ones run. With q / k norm weights 1 + U(0.5) hd16 stands 13.6 tolerances
off; hd128_gqa stood 9.6 off (its two precisions are 0.07 apart, so its tolerance is 0.22) and takes synth_qwen3_state's
default spread 0.75: 14.8."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from llamarec_amd.synth import synth_qwen3_state
from tests.gen_goldens_gemma import save_npz_fixed
from tests.gen_goldens_gemma2 import golden_tolerance  # noqa: F401  (the GPU test's bound; re-exported)

QWEN3_CONFIGS = {
    # name: (vocab, hidden, inter, layers, heads, kv_heads, head_dim, tied head, weight width, q/k norm spread)
    "hd128_gqa": (320, 256, 512, 2, 4, 2, 128, True, 0.02, 0.75),   # nh * hd = 512 != hidden; the MFMA kernels
    "hd16": (320, 64, 128, 2, 4, 2, 16, True, 0.07, 0.5),           # the generic kernels
}
LABEL_IDS = list(range(40, 60))
LENS = [37, 5, 64, 1, 20, 130]


def qwen3_cfg_dict(name):
    v, d, f, nl, nh, nkv, hd, tied, _, _ = QWEN3_CONFIGS[name]
    return dict(model_type="qwen3", vocab_size=v, hidden_size=d, intermediate_size=f, num_hidden_layers=nl,
                num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd, max_position_embeddings=256, rms_norm_eps=1e-6,
                rope_theta=1000000.0, rope_scaling=None, hidden_act="silu", attention_bias=False, use_sliding_window=False,
                sliding_window=None, max_window_layers=nl, tie_word_embeddings=tied)


def hf_model(cd, sd):
    from transformers import Qwen3Config, Qwen3ForCausalLM

    kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta", "rope_scaling")}
    kw.update(attention_dropout=0.0, pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="eager")
    try:
        cfg = Qwen3Config(**kw, rope_parameters={"rope_type": "default", "rope_theta": cd["rope_theta"]})
    except TypeError:
        cfg = Qwen3Config(**kw, rope_theta=cd["rope_theta"], rope_scaling=None)
    model = Qwen3ForCausalLM(cfg).eval()
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    allowed = ("rotary",) + (("lm_head.weight",) if cd["tie_word_embeddings"] else ())
    assert not [k for k in missing.missing_keys if not any(a in k for a in allowed)], missing
    assert not missing.unexpected_keys, missing
    if cd["tie_word_embeddings"] and model.lm_head.weight.data_ptr() != model.model.embed_tokens.weight.data_ptr():
        model.lm_head.weight = model.model.embed_tokens.weight
    att = model.model.layers[0].self_attn
    assert att.q_norm.weight.shape == (cd["head_dim"],) and att.q_proj.bias is None
    assert att.q_proj.weight.shape == (cd["num_attention_heads"] * cd["head_dim"], cd["hidden_size"])
    return model


def last_logits_hf(model, ids, mask):
    """logits[:, -1].float() of a left-padded batch, positions counted from each prompt's first token"""
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    return model(input_ids=ids, attention_mask=mask, position_ids=pos).logits[:, -1].float().numpy()


def main(REF, OUT):
    from tests import qwen3_ref as QR

    torch.manual_seed(0)
    for ci, name in enumerate(QWEN3_CONFIGS):
        cd = qwen3_cfg_dict(name)
        seed = 700 + ci
        std, spread = QWEN3_CONFIGS[name][-2:]
        sd = synth_qwen3_state(cd, seed, std=std, qk_norm_spread=spread)
        model = hf_model(cd, sd)
        rng = np.random.default_rng(seed)
        T = max(LENS)
        ids = np.zeros((len(LENS), T), np.int64)
        mask = np.zeros((len(LENS), T), np.int64)
        for b, n in enumerate(LENS):
            ids[b, T - n:] = rng.integers(3, cd["vocab_size"], size=n)
            ids[b, T - n] = 1   # <s>
            mask[b, T - n:] = 1
        tids, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
        ones = {k: (np.ones_like(v) if k.endswith(("q_norm.weight", "k_norm.weight")) else v) for k, v in sd.items()}
        with torch.no_grad():
            l32 = last_logits_hf(model, tids, tmask)
            lun = np.stack([model(input_ids=tids[b:b + 1, T - n:]).logits[0, -1].float().numpy() for b, n in enumerate(LENS)])
            l_ones = last_logits_hf(hf_model(cd, ones), tids, tmask)
            lbf = last_logits_hf(model.to(torch.bfloat16), tids, tmask)
        assert l32.shape == (len(LENS), cd["vocab_size"])
        tol = golden_tolerance(l32, lbf)
        seqs = [ids[b, T - n:] for b, n in enumerate(LENS)]
        restated = QR.last_logits(sd, cd, seqs)
        restated_ones = QR.last_logits(sd, cd, seqs, mutant="ones_norm")
        moved = float(np.abs(l_ones - l32).max())
        print(f"{name}: max |logit| {np.abs(l32).max():.3f}, bf16-fp32 {np.abs(lbf - l32).max():.4f}, tolerance {tol:.4f}, "
              f"restatement-fp32 {np.abs(restated - l32).max():.2e}, padded-unpadded {np.abs(lun - l32).max():.2e}, "
              f"q/k norm weights of ones {moved:.3f} ({moved / tol:.1f} tolerances)")
        scale = max(1.0, np.abs(l32).max())
        assert np.abs(restated - l32).max() < 1e-3 * scale and np.abs(restated_ones - l_ones).max() < 1e-3 * scale
        assert moved > 10 * tol, f"{name}: norm weights of ones move logits_fp32 by {moved}, not ten times the tolerance {tol}"
        save_npz_fixed(os.path.join(OUT, f"qwen3_tiny_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(seed), weight_std=np.array(std), qk_norm_spread=np.array(spread), input_ids=ids,
                       attention_mask=mask, lens=np.array(LENS), logits_fp32=l32, logits_fp32_unpadded=lun, logits_bf16=lbf,
                       eval_loss=np.array(-1.0), label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS],
                       scores_bf16=lbf[:, LABEL_IDS])


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_qwen3 <reference tree> [out dir]")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out)
