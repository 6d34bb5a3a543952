"""Qwen2 goldens (tests/golden/qwen2_tiny_*.npz): runs the reference's Qwen2ForCausalLMPatched (model/llm.py:570-672, eager
attention) in fp32 and bf16 on tiny configs whose weights synth_qwen2_state rebuilds from a seed, and stores data only -- the
keys of phi3_tiny_*.npz plus bias_std and v_bias_std. Run on a CPU machine with the reference tree:
    python -m tests.gen_goldens_qwen2 <reference dir> [out dir]
The archives are written with fixed zip timestamps (save_npz_fixed), so a rerun reproduces them byte for byte.

Before a file is written the generator asserts that the goldens are Qwen2's own: dropping the q/k/v biases, or leaving the q and
k biases in HF's order while the weight rows are pair-interleaved, must move logits_fp32 by at least ten times the tolerance
the GPU test holds the prefill to (golden_tolerance, computed from the archive's own two precisions). Both misreadings are
evaluated with the fp32 restatement tests/qwen2_ref.py, which must itself sit on the reference's fp32 logits. The q and k biases
have synth_qwen2_state's default width 0.5 (the published checkpoints' reach several units), the v bias 0.1 (V_BIAS_STD).
With a v bias of 0.5 too, beside weights of width 0.02, every position's value is nearly the same vector, the attention
weights hardly reach the logits and the HF-order misreading -- which acts on the scores alone -- moved logits_fp32 by
0.11 .. 0.22 (4 .. 7 tolerances) at EVERY q/k width from 0.15 to 2.5: widening the biases does not help, narrowing v's does
(0.44 .. 1.04 at 0.5 / 0.1). hd128_gqa, the smallest of those, also takes q/k biases 1.0 wide (1.00)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from llamarec_amd.synth import synth_qwen2_state
from tests.gen_goldens_gemma import save_npz_fixed
from tests.gen_goldens_gemma2 import golden_tolerance  # noqa: F401  (the GPU test's bound; re-exported)

QWEN2_CONFIGS = {
    # name: (vocab, hidden, inter, layers, heads, kv_heads, tied head, weight width, bias width)
    "hd64_ragged": (320, 896, 1280, 2, 14, 2, True, 0.02, 0.5),    # Qwen2-0.5B's widths: qkv 1152, o / down 896 ragged; GQA group 7
    "hd128_gqa": (320, 512, 1024, 2, 4, 2, False, 0.02, 1.0),      # the bias on the 256-column tile's own instantiation
    "hd16": (320, 64, 128, 2, 4, 2, True, 0.07, 0.5),              # the generic kernels
}
V_BIAS_STD = 0.1
LABEL_IDS = list(range(40, 60))
LENS = [37, 5, 64, 1, 20, 130]


def qwen2_cfg_dict(name):
    v, d, f, nl, nh, nkv, tied, _, _ = QWEN2_CONFIGS[name]
    return dict(model_type="qwen2", vocab_size=v, hidden_size=d, intermediate_size=f, num_hidden_layers=nl,
                num_attention_heads=nh, num_key_value_heads=nkv, max_position_embeddings=256, rms_norm_eps=1e-6,
                rope_theta=1000000.0, hidden_act="silu", use_sliding_window=False, sliding_window=256, max_window_layers=nl,
                tie_word_embeddings=tied)


def hf_model(cd, sd):
    from transformers import Qwen2Config, Qwen2ForCausalLM

    kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta")}
    kw.update(attention_dropout=0.0, pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="eager")
    try:
        cfg = Qwen2Config(**kw, rope_parameters={"rope_type": "default", "rope_theta": cd["rope_theta"]})
    except TypeError:
        cfg = Qwen2Config(**kw, rope_theta=cd["rope_theta"], rope_scaling=None)
    model = Qwen2ForCausalLM(cfg).eval()
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    allowed = ("rotary",) + (("lm_head.weight",) if cd["tie_word_embeddings"] else ())
    assert not [k for k in missing.missing_keys if not any(a in k for a in allowed)], missing
    assert not missing.unexpected_keys, missing
    tied = model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    if cd["tie_word_embeddings"] and not tied:
        model.lm_head.weight = model.model.embed_tokens.weight
    assert (model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()) == cd["tie_word_embeddings"]
    assert model.model.layers[0].self_attn.q_proj.bias is not None and model.model.layers[0].self_attn.o_proj.bias is None
    return model


def main(REF, OUT):
    sys.path.insert(0, REF)
    import model.llm as ML  # noqa: F401  (patches Qwen2ForCausalLM.forward at import, model/llm.py:672)

    from tests import qwen2_ref as QR

    torch.manual_seed(0)
    for ci, name in enumerate(QWEN2_CONFIGS):
        cd = qwen2_cfg_dict(name)
        seed = 600 + ci
        std, bias_std = QWEN2_CONFIGS[name][-2:]
        sd = synth_qwen2_state(cd, seed, std=std, bias_std=bias_std, v_bias_std=V_BIAS_STD)
        model = hf_model(cd, sd)
        rng = np.random.default_rng(seed)
        T = max(LENS)
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
        restated = QR.last_logits(sd, cd, seqs)
        moved = {m: float(np.abs(QR.last_logits(sd, cd, seqs, mutant=m) - l32).max()) for m in QR.QWEN2_MUTANTS}
        print(f"{name}: max |logit| {np.abs(l32).max():.3f}, bf16-fp32 {np.abs(lbf - l32).max():.4f}, tolerance {tol:.4f}, "
              f"restatement-fp32 {np.abs(restated - l32).max():.2e}, biases dropped {moved['no_bias']:.3f}, "
              f"q/k biases in HF order {moved['hf_order_bias']:.3f}")
        assert np.abs(restated - l32).max() < 1e-3 * max(1.0, np.abs(l32).max())
        for m, dist in moved.items():
            assert dist >= 10 * tol, f"{name}: the {m} misreading moves logits_fp32 by {dist}, less than ten times the tolerance {tol}"
        save_npz_fixed(os.path.join(OUT, f"qwen2_tiny_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(seed), weight_std=np.array(std), bias_std=np.array(bias_std), v_bias_std=np.array(V_BIAS_STD), input_ids=ids,
                       attention_mask=mask, lens=np.array(LENS), logits_fp32=l32, logits_fp32_unpadded=lun, logits_bf16=lbf,
                       eval_loss=np.array(loss), label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS],
                       scores_bf16=lbf[:, LABEL_IDS])


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_qwen2 <reference tree> [out dir]")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out)
