"""Gemma-3 goldens (tests/golden/gemma3_tiny_*.npz): runs tests/gemma3_ref.py -- the torch restatement of HF's
Gemma3ForCausalLM (text) -- in fp32 and bf16 on tiny configs whose weights synth_gemma3_state rebuilds from a seed, and stores
data only: the prompts, logits_fp32, logits_bf16 and the fp32 logits of every mutant of the reference (gemma3_ref.MODEL_MUTANTS).
Where the installed transformers has Gemma3ForCausalLM the generator first checks the restatement against it (eager attention,
fp32, one prompt at a time) and refuses to write anything on a disagreement. Run on a CPU machine:
    python -m tests.gen_goldens_gemma3 [out dir]
The archives are written with fixed zip timestamps (save_npz_fixed), so a rerun reproduces them byte for byte.

With 0.02-wide weights a tiny model's logits are about 0.1 and one key more or less at a window's edge would be invisible, so
each config picks its weight width, its q/k norm weights (their mean makes the attention peaked), the weight of its attention
branch and its window such that the mutants matter: the generator refuses to write a file unless each mutant's logits (but
WEAK_MUTANTS, below) are at least ten times the tolerance the GPU test holds the prefill to (golden_tolerance below, computed
from the archive's own two precisions) away from logits_fp32."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from llamarec_amd.synth import synth_gemma3_state
from tests import gemma3_ref as G3
from tests.gen_goldens_gemma import save_npz_fixed

SLIDING, FULL = "sliding_attention", "full_attention"
GEMMA3_CONFIGS = {
    # name: (config overrides, synth_gemma3_state's knobs, prompt lengths)
    # gemma-3-1b's attention shape: MQA at head_dim 256; hidden 320 is a multiple of 64 but not of 256; 7 layers of pattern 6, so
    # layer 5 is global and the last layer sliding; prompts from under the window of 100 to about three windows. The last two
    # layers (the global one and a sliding one) are peaked, the five in front of them flat.
    "tiny_hd256_mqa": (dict(hidden_size=320, intermediate_size=512, num_hidden_layers=7, num_attention_heads=4,
                            num_key_value_heads=1, head_dim=256, query_pre_attn_scalar=256, sliding_window=100,
                            sliding_window_pattern=6),
                       dict(std=0.06, qk_norm_mean=[-0.4] * 5 + [1.0, 1.0], attn_out_mean=2.0, mlp_out_mean=-0.9),
                       [37, 100, 101, 5, 250, 1, 310, 130]),
    # the generic attention route: head_dim 128, GQA, layer kinds spelled out, a window of 8 keys
    "tiny_hd128": (dict(hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=4,
                        num_key_value_heads=2, head_dim=128, query_pre_attn_scalar=128, sliding_window=8,
                        layer_types=[SLIDING, FULL, SLIDING]),
                   dict(std=0.06, qk_norm_mean=0.0, attn_out_mean=2.0, mlp_out_mean=-0.9), [5, 8, 9, 1, 30, 20, 17, 70]),
    # rope_scaling linear on the global layers (the larger Gemma-3 text models: factor 8), head_dim 256, a window of 8 keys
    "tiny_hd256_linear": (dict(hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                               num_key_value_heads=1, head_dim=256, query_pre_attn_scalar=256, sliding_window=8,
                               layer_types=[SLIDING, FULL, SLIDING], rope_scaling={"rope_type": "linear", "factor": 8.0}),
                          dict(std=0.06, qk_norm_mean=0.0, attn_out_mean=2.0, mlp_out_mean=-0.9),
                          [5, 8, 9, 1, 30, 20, 17, 140]),
}
# Mutants an archive cannot show at ten tolerances, with the reason. One key more or less in a window of W keys moves a flat
# attention row's output by about 1 / sqrt(W) of its size -- 10 % at W = 100 -- and the logits by less, while the reference's
# own bf16 run sits 0.7 % of the logit scale from its fp32 run (so ten tolerances are 21 %); peaked scores raise both sides
# alike. Measured over 30 settings of the knobs and three seeds: 1.0 .. 5.3 tolerances, never 10. The window's edge at the
# model level is therefore shown by the two archives with a window of 8 keys (and, per key, by the kernel tests).
WEAK_MUTANTS = {"tiny_hd256_mqa": ("window_plus_one", "window_minus_one")}
LABEL_IDS = list(range(40, 60))
PREFILL_TOL = 3e-2      # Gemma v1's bound on the prefill against its goldens


def golden_tolerance(logits_fp32, logits_bf16):
    """The GPU test's bound for an archive (tests/gen_goldens_gemma2.py's rule, restated): Gemma v1's 3e-2 while the reference's
    own two precisions agree to a third of it, otherwise three times their distance."""
    gap = float(np.abs(np.asarray(logits_bf16) - np.asarray(logits_fp32)).max())
    return PREFILL_TOL if gap <= PREFILL_TOL / 3 else 3.0 * gap


def gemma3_cfg_dict(name):
    over = GEMMA3_CONFIGS[name][0]
    return dict(dict(model_type="gemma3_text", vocab_size=320, max_position_embeddings=1024, rms_norm_eps=1e-6,
                     rope_theta=1000000.0, rope_local_base_freq=10000.0, rope_scaling=None,
                     hidden_activation="gelu_pytorch_tanh", attn_logit_softcapping=None, final_logit_softcapping=None,
                     attention_bias=False), **over)


def golden_state(name, seed):
    return synth_gemma3_state(gemma3_cfg_dict(name), seed, **GEMMA3_CONFIGS[name][1])


def hf_logits(cd, sd, seqs):
    """fp32 last-token logits of transformers' Gemma3ForCausalLM (eager attention), or None when it is not installed."""
    try:
        from transformers import Gemma3ForCausalLM, Gemma3TextConfig
    except ImportError:
        return None
    sliding = G3.layer_is_sliding(cd)
    kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta", "rope_local_base_freq", "rope_scaling",
                                                    "sliding_window_pattern", "layer_types")}
    g = {"rope_type": "default", "rope_theta": cd["rope_theta"]}
    if cd.get("rope_scaling"):
        g = {"rope_type": "linear", "factor": cd["rope_scaling"]["factor"], "rope_theta": cd["rope_theta"]}
    cfg = Gemma3TextConfig(**kw, layer_types=[SLIDING if s else FULL for s in sliding],
                           rope_parameters={FULL: g, SLIDING: {"rope_type": "default", "rope_theta": cd["rope_local_base_freq"]}},
                           tie_word_embeddings=True, attn_implementation="eager")
    model = Gemma3ForCausalLM(cfg).eval()
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not [k for k in missing.missing_keys if "rotary" not in k and k != "lm_head.weight"], missing
    assert not missing.unexpected_keys, missing
    with torch.no_grad():
        return np.stack([model(input_ids=torch.from_numpy(np.asarray(s, np.int64))[None]).logits[0, -1].float().numpy()
                         for s in seqs])


def main(OUT):
    torch.manual_seed(0)
    for ci, name in enumerate(GEMMA3_CONFIGS):
        cd = gemma3_cfg_dict(name)
        lens = GEMMA3_CONFIGS[name][2]
        seed = 700 + ci
        sd = golden_state(name, seed)
        rng = np.random.default_rng(seed)
        seqs = [np.concatenate([[2], rng.integers(3, cd["vocab_size"], size=n - 1)]).astype(np.int64) for n in lens]   # <bos>
        l32 = G3.last_logits(sd, cd, seqs, torch.float32)
        lbf = G3.last_logits(sd, cd, seqs, torch.bfloat16)
        hf = hf_logits(cd, sd, seqs)
        if hf is not None:
            d = float(np.abs(hf - l32).max())
            print(f"{name}: transformers' Gemma3ForCausalLM agrees with the restatement to {d:.2e}")
            assert d < 1e-3, (name, d)
        tol = golden_tolerance(l32, lbf)
        mut = {m: G3.last_logits(sd, cd, seqs, torch.float32, mutant=m) for m in G3.MODEL_MUTANTS}
        moved = {m: float(np.abs(v - l32).max()) for m, v in mut.items()}
        print(f"{name}: max |logit| {np.abs(l32).max():.3f}, bf16-fp32 {np.abs(lbf - l32).max():.4f}, tolerance {tol:.4f}, mutants "
              + ", ".join(f"{m} {d:.3f}" for m, d in moved.items()))
        for m, d in moved.items():
            if m in WEAK_MUTANTS.get(name, ()):
                continue
            assert d >= 10 * tol, f"{name}: mutant {m} moves logits_fp32 by {d}, less than ten times the tolerance {tol}"
        ids = np.concatenate(seqs)
        save_npz_fixed(os.path.join(OUT, f"gemma3_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(seed), input_ids=ids, lens=np.array(lens), logits_fp32=l32, logits_bf16=lbf,
                       label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS], scores_bf16=lbf[:, LABEL_IDS],
                       **{f"mutant_{m}": v for m, v in mut.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
