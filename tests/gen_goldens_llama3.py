"""Llama-3.1 / 3.2 goldens (tests/golden/llama3_tiny_*.npz): runs the reference's LlamaForCausalLMPatched (model/llm.py:35-145,
eager attention) with rope_scaling = llama3 in fp32 and bf16 on tiny configs whose weights synth_llama_state rebuilds from a
seed, and stores data only -- the keys of gemma_tiny_*.npz plus
  logits_fp32_plain_rope  the same weights and inputs with rope_type default: what a loader that ignored rope_scaling gives
  bf16_gap                max |logits_bf16 - logits_fp32|, the model's own rounding distance (the tests' tolerance unit)
  weight_std
The scaling (factor 8, low 1, high 4, original_max_position_embeddings 64, rope_theta 500000) exercises all three branches
of the rule: at head_dim 64, frequencies 0-2 are unchanged, 3-5 interpolated, the rest divided by 8. WEIGHT_STD = 0.04: with
synth_llama_state's default 0.02 the attention is nearly uniform and scaled and plain RoPE differ by about as much as bf16
and fp32 do, so a golden would not tell them apart; the generator asserts the plain-vs-scaled gap is >= 8 bf16_gap for every
prompt of at least 20 tokens (SEED = 403: the smallest ratio is 11.3 at head_dim 64 and 11.6 at head_dim 128; seeds 400 to
402 leave one prompt at 6 to 7 and are refused by that assertion).
Run on a CPU machine with the reference tree:  python -m tests.gen_goldens_llama3 <reference dir> [out dir]. The archives
are written with fixed zip timestamps, so a rerun reproduces them byte for byte."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from llamarec_amd.synth import synth_llama_state
from tests.gen_goldens_gemma import save_npz_fixed

LLAMA3_CONFIGS = {
    # name: (vocab, hidden, inter, layers, heads, kv_heads, head_dim, tied)
    "tiny_hd64_gqa": (320, 256, 512, 2, 4, 2, 64, True),    # Llama-3.2-1B's attention shape: GQA at head_dim 64, tied head
    "tiny_hd128": (320, 256, 512, 2, 2, 2, 128, False),     # Llama-3.1-8B's head_dim
}
ROPE_SCALING = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                    original_max_position_embeddings=64)
LABEL_IDS = list(range(40, 60))
LENS = [37, 5, 64, 1, 20, 130, 300]
WEIGHT_STD = 0.04
SEED = 403


def llama3_cfg_dict(name):
    v, d, f, nl, nh, nkv, hd, tied = LLAMA3_CONFIGS[name]
    return dict(model_type="llama", vocab_size=v, hidden_size=d, intermediate_size=f, num_hidden_layers=nl,
                num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd, max_position_embeddings=512,
                rms_norm_eps=1e-5, rope_theta=500000.0, tie_word_embeddings=tied, rope_scaling=dict(ROPE_SCALING))


def llama3_state(name, seed=SEED):
    """The golden's weights: synth_llama_state at WEIGHT_STD, without lm_head.weight when the config ties it."""
    cd = llama3_cfg_dict(name)
    sd = synth_llama_state(cd, seed, std=WEIGHT_STD)
    if cd["tie_word_embeddings"]:
        del sd["lm_head.weight"]
    return sd


def main(REF, OUT):
    sys.path.insert(0, REF)
    import model.llm as ML  # noqa: F401  (patches LlamaForCausalLM.forward at import, model/llm.py:145)
    from transformers import LlamaConfig, LlamaForCausalLM

    def build(cd, scaled):
        kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta", "rope_scaling")}
        rp = dict(ROPE_SCALING) if scaled else {"rope_type": "default"}
        try:
            cfg = LlamaConfig(**kw, rope_parameters=dict(rp, rope_theta=cd["rope_theta"]), attention_bias=False, mlp_bias=False,
                              attn_implementation="eager")
        except TypeError:
            cfg = LlamaConfig(**kw, rope_theta=cd["rope_theta"], rope_scaling=rp if scaled else None, attention_bias=False,
                              mlp_bias=False, attn_implementation="eager")
        return LlamaForCausalLM(cfg).eval()

    torch.manual_seed(0)
    for name in LLAMA3_CONFIGS:
        cd = llama3_cfg_dict(name)
        sd = llama3_state(name)
        tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
        model, plain = build(cd, True), build(cd, False)
        for m in (model, plain):
            missing = m.load_state_dict(tsd, strict=False)
            allowed = ("lm_head.weight",) if cd["tie_word_embeddings"] else ()
            assert not [k for k in missing.missing_keys if "rotary" not in k and k not in allowed], missing
            assert torch.equal(m.lm_head.weight, m.model.embed_tokens.weight) == cd["tie_word_embeddings"]
        assert not torch.equal(model.model.rotary_emb.inv_freq, plain.model.rotary_emb.inv_freq)
        rng = np.random.default_rng(SEED)
        lens = LENS
        T = max(lens)
        ids = np.zeros((len(lens), T), np.int64)
        mask = np.zeros((len(lens), T), np.int64)
        for b, n in enumerate(lens):
            ids[b, T - n:] = rng.integers(3, cd["vocab_size"], size=n)
            ids[b, T - n] = 1   # <s>
            mask[b, T - n:] = 1
        labels = np.zeros((len(lens), 1), np.int64)
        tid, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
        with torch.no_grad():
            o32 = model(input_ids=tid, attention_mask=tmask, labels=torch.from_numpy(labels))
            loss = float(o32.loss)
            l32 = o32.logits.numpy()
            lplain = plain(input_ids=tid, attention_mask=tmask).logits.numpy()
            lun = np.stack([model(input_ids=tid[b:b + 1, T - n:]).logits[0].numpy() for b, n in enumerate(lens)])
            mb = model.to(torch.bfloat16)
            lbf = mb(input_ids=tid, attention_mask=tmask).logits
            assert lbf.dtype == torch.float32
            lbf = lbf.numpy()
        assert l32.shape == (len(lens), cd["vocab_size"]) and loss == -1.0
        gap = float(np.abs(lbf - l32).max())
        for b, n in enumerate(lens):
            d = float(np.abs(lplain[b] - l32[b]).max())
            print(f"llama3_{name}: prompt of {n:3d} tokens  plain-vs-scaled {d:.4f}  = {d / gap:.1f} x bf16_gap {gap:.4f}")
            if n >= 20:
                assert d >= 8 * gap, (name, n, d, gap)
        save_npz_fixed(os.path.join(OUT, f"llama3_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(SEED), weight_std=np.array(WEIGHT_STD), input_ids=ids, attention_mask=mask,
                       lens=np.array(lens), logits_fp32=l32, logits_fp32_unpadded=lun, logits_bf16=lbf,
                       logits_fp32_plain_rope=lplain, bf16_gap=np.array(gap), eval_loss=np.array(loss),
                       label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS], scores_bf16=lbf[:, LABEL_IDS])


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_llama3 <reference tree> [out dir]")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out)
