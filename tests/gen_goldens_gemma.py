"""Gemma goldens (tests/golden/gemma_tiny_*.npz): runs the reference's GemmaForCausalLMPatched (model/llm.py:354-456,
eager attention) in fp32 and bf16 on tiny configs whose weights synth_gemma_state rebuilds from a seed, and stores data
only -- the keys of llama_tiny_*.npz plus the verbalizer scores of LABEL_IDS. Run on a CPU machine with the reference
tree:  python -m tests.gen_goldens_gemma <reference dir> [out dir]. The archives are written with fixed zip timestamps,
so a rerun reproduces them byte for byte."""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

from llamarec_amd.synth import synth_gemma_state

GEMMA_CONFIGS = {
    # name: (vocab, hidden, inter, layers, heads, kv_heads, head_dim)
    "tiny_hd256_mqa": (320, 256, 512, 2, 4, 1, 256),   # gemma-2b's attention shape: MQA at head_dim 256
    "tiny_hd256_wide": (320, 256, 512, 2, 2, 2, 256),  # gemma-7b's: nh * hd = 512 != hidden 256
    "tiny_hd16": (320, 64, 128, 2, 4, 2, 16),          # the generic attention kernel
}
LABEL_IDS = list(range(40, 60))


def gemma_cfg_dict(name):
    v, d, f, nl, nh, nkv, hd = GEMMA_CONFIGS[name]
    return dict(model_type="gemma", vocab_size=v, hidden_size=d, intermediate_size=f, num_hidden_layers=nl,
                num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd, max_position_embeddings=256,
                rms_norm_eps=1e-6, rope_theta=10000.0, hidden_activation="gelu_pytorch_tanh")


def save_npz_fixed(path, **arrays):
    """np.savez_compressed with a fixed timestamp on every member (byte-reproducible)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def main(REF, OUT):
    sys.path.insert(0, REF)
    import model.llm as ML  # noqa: F401  (patches GemmaForCausalLM.forward at import, model/llm.py:454)
    from transformers import GemmaConfig, GemmaForCausalLM

    torch.manual_seed(0)
    for ci, name in enumerate(GEMMA_CONFIGS):
        cd = gemma_cfg_dict(name)
        kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta")}
        try:
            cfg = GemmaConfig(**kw, rope_parameters={"rope_type": "default", "rope_theta": cd["rope_theta"]},
                              attention_bias=False, tie_word_embeddings=True, attn_implementation="eager")
        except TypeError:
            cfg = GemmaConfig(**kw, rope_theta=cd["rope_theta"], attention_bias=False, tie_word_embeddings=True,
                              attn_implementation="eager")
        seed = 300 + ci
        sd = synth_gemma_state(cd, seed)
        model = GemmaForCausalLM(cfg).eval()
        missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not [k for k in missing.missing_keys if "rotary" not in k and k != "lm_head.weight"], missing
        assert torch.equal(model.lm_head.weight, model.model.embed_tokens.weight)   # tied
        rng = np.random.default_rng(seed)
        lens = [37, 5, 64, 1, 20, 130]
        T = max(lens)
        ids = np.zeros((len(lens), T), np.int64)
        mask = np.zeros((len(lens), T), np.int64)
        for b, n in enumerate(lens):
            ids[b, T - n:] = rng.integers(3, cd["vocab_size"], size=n)
            ids[b, T - n] = 2   # <bos> of the Gemma tokenizer
            mask[b, T - n:] = 1
        labels = np.zeros((len(lens), 1), np.int64)
        with torch.no_grad():
            o32 = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask),
                        labels=torch.from_numpy(labels))
            loss = float(o32.loss)
            l32 = o32.logits.numpy()
            lun = np.stack([model(input_ids=torch.from_numpy(ids[b:b + 1, T - n:])).logits[0].numpy()
                            for b, n in enumerate(lens)])
            mb = model.to(torch.bfloat16)
            lbf = mb(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).logits
            assert lbf.dtype == torch.float32
            lbf = lbf.numpy()
        assert l32.shape == (len(lens), cd["vocab_size"]) and loss == -1.0
        save_npz_fixed(os.path.join(OUT, f"gemma_{name}.npz"), config=np.array(json.dumps(cd, sort_keys=True)),
                       weight_seed=np.array(seed), input_ids=ids, attention_mask=mask, lens=np.array(lens),
                       logits_fp32=l32, logits_fp32_unpadded=lun, logits_bf16=lbf, eval_loss=np.array(loss),
                       label_ids=np.array(LABEL_IDS), scores_fp32=l32[:, LABEL_IDS], scores_bf16=lbf[:, LABEL_IDS])


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_gemma <reference tree> [out dir]")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out)
