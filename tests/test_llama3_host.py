"""CPU: the Llama-3.1 / 3.2 ranker's host side -- the torch restatement (llama3 RoPE scaling) against the reference's goldens,
rope_scaling / rope_parameters parsing, the presets, the new ABI struct and symbols, and the build-time ISA checks of the
head_dim-64 attention TU."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "llamarec_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LLAMA3_GOLDENS = ("tiny_hd64_gqa", "tiny_hd128")
LLAMA3 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)
# The occupancy plan of DESIGN section 10: three workgroups (12 waves) per CU need <= 512 / 3 = 170 registers per lane, in
# the allocation granule of 8: 168.
HD64_VGPR_BOUND = 168


def load_llama3_golden(golden_dir, name):
    """(archive, config dict, state dict rebuilt from the seed, unpadded prompts)."""
    from llamarec_amd.synth import synth_llama_state

    z = np.load(os.path.join(golden_dir, f"llama3_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_llama_state(cfg, int(z["weight_seed"]), std=float(z["weight_std"]))
    if cfg["tie_word_embeddings"]:
        del sd["lm_head.weight"]
    T = z["input_ids"].shape[1]
    seqs = [z["input_ids"][b, T - n:] for b, n in enumerate(z["lens"])]
    return z, cfg, sd, seqs


@pytest.mark.parametrize("name", LLAMA3_GOLDENS)
def test_llama3_restatement_matches_reference_goldens(golden_dir, name):
    from tests import llama3_ref as R

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, name)
    gap = float(z["bf16_gap"])
    assert cfg["rope_scaling"]["rope_type"] == "llama3" and cfg["head_dim"] in (64, 128) and 0.005 < gap < 0.1
    assert ("lm_head.weight" in sd) == (not cfg["tie_word_embeddings"])
    l32 = R.last_logits(sd, cfg, seqs)
    assert np.abs(l32 - z["logits_fp32"]).max() < 1e-4
    assert np.abs(l32 - z["logits_fp32_unpadded"]).max() < 1e-4
    lbf = R.last_logits(sd, cfg, seqs, torch.bfloat16)
    assert np.abs(lbf - z["logits_bf16"]).max() < 4 * gap
    assert np.array_equal(z["scores_bf16"], z["logits_bf16"][:, z["label_ids"]])
    # the goldens really are scaled RoPE: the plain table reproduces the reference's plain run and is far from the scaled one
    lplain = R.last_logits(sd, cfg, seqs, scaled=False)
    assert np.abs(lplain - z["logits_fp32_plain_rope"]).max() < 1e-4
    long = np.nonzero(z["lens"] >= 20)[0]
    assert len(long) >= 5
    assert np.abs(lplain - z["logits_fp32"])[long].max(axis=1).min() > 2 * gap
    # all three branches of the rule are taken
    inv = R.llama3_inv_freq(cfg["head_dim"], cfg["rope_theta"], cfg["rope_scaling"]).numpy()
    ratio = R.llama3_inv_freq(cfg["head_dim"], cfg["rope_theta"], None).numpy() / inv
    assert (ratio == 1).any() and np.isclose(ratio, 8).any() and ((ratio > 1.001) & (ratio < 7.999)).any()
    if cfg["head_dim"] == 64:
        assert (ratio[:3] == 1).all() and ((ratio[3:6] > 1) & (ratio[3:6] < 8)).all() and np.allclose(ratio[6:], 8)


def test_model_family_accepts_llama3_scaling_in_both_layouts():
    from llamarec_amd.llm import GEMMA_2B, LLAMA2_7B, LlamaRanker, model_family, rope_parameters

    hf4 = dict(LLAMA2_7B, model_type="llama", rope_theta=500000.0, rope_scaling=dict(LLAMA3))
    hf5 = dict({k: v for k, v in LLAMA2_7B.items() if k != "rope_theta"}, model_type="llama",
               rope_parameters=dict(LLAMA3, rope_theta=500000.0))
    legacy = dict(hf4, rope_scaling=dict({k: v for k, v in LLAMA3.items() if k != "rope_type"}, type="llama3"))
    numbers = {k: v for k, v in LLAMA3.items() if k != "rope_type"}
    for c in (hf4, hf5, legacy):
        assert model_family(c) == "llama"
        assert rope_parameters(c) == (500000.0, numbers)
        r = LlamaRanker(c, device="cpu")
        assert r.rope_theta == 500000.0 and r.rope_scaling == numbers
    for plain in (dict(LLAMA2_7B), dict(LLAMA2_7B, rope_scaling=None), dict(LLAMA2_7B, rope_scaling={"rope_type": "default"}),
                  dict(LLAMA2_7B, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})):
        assert model_family(plain) == "llama" and rope_parameters(plain) == (10000.0, None)
    for missing in numbers:
        bad = dict(hf4, rope_scaling={k: v for k, v in LLAMA3.items() if k != missing})
        with pytest.raises(NotImplementedError, match="rope_scaling"):
            model_family(bad)
        bad5 = dict(hf5, rope_parameters={k: v for k, v in hf5["rope_parameters"].items() if k != missing})
        with pytest.raises(NotImplementedError, match="rope_scaling"):
            model_family(bad5)
    for kind in ("yarn", "linear", "dynamic", "longrope"):
        with pytest.raises(NotImplementedError, match="rope_scaling"):
            model_family(dict(hf4, rope_scaling={"rope_type": kind, "factor": 2.0}))
        with pytest.raises(NotImplementedError, match="rope_scaling"):
            model_family(dict(hf4, rope_scaling={"type": kind, "factor": 2.0}))
    with pytest.raises(NotImplementedError, match="rope_scaling"):
        model_family(dict(GEMMA_2B, rope_scaling=dict(LLAMA3)))
    with pytest.raises(NotImplementedError, match="rope_scaling"):
        model_family(dict(LLAMA2_7B, model_type="mistral", rope_scaling={"rope_type": "yarn", "factor": 4.0}))


def test_llama3_presets():
    from llamarec_amd.llm import LLAMA31_8B, LLAMA32_1B, LLAMA32_3B, LlamaRanker
    from llamarec_amd import config as cfg

    want = {"1b": (LLAMA32_1B, 64, 4, 2048, 16, 32.0, True), "3b": (LLAMA32_3B, 128, 3, 3072, 28, 32.0, True),
            "8b": (LLAMA31_8B, 128, 4, 4096, 32, 8.0, False)}
    for c, hd, gqa, d, layers, factor, tied in want.values():
        r = LlamaRanker(c, device="cpu")
        assert r.family == "llama" and r.hd == hd == c["head_dim"]
        assert c["num_attention_heads"] // c["num_key_value_heads"] == gqa and c["num_key_value_heads"] == 8
        assert (c["hidden_size"], c["num_hidden_layers"], c["vocab_size"]) == (d, layers, 128256)
        assert r.rope_theta == 500000.0 and r.rope_scaling["factor"] == factor
        assert r.rope_scaling["original_max_position_embeddings"] == 8192 and c["max_position_embeddings"] == 131072
        assert bool(c["tie_word_embeddings"]) == tied
        # every GEMM shape is a multiple of the 256 x 256 x 64 tile
        qkv = (c["num_attention_heads"] + 2 * c["num_key_value_heads"]) * hd
        assert all(n % 256 == 0 for n in (qkv, d, 2 * c["intermediate_size"])) and d % 64 == 0 and c["intermediate_size"] % 64 == 0
    assert "llama3" in cfg.LLM_CHOICES


def test_rope_scaling_abi(tmp_path):
    from llamarec_amd import _abi as A
    from llamarec_amd import _lib

    l = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("lr_llama_set_rope_scaling", "lr_rope_table_ex"):
        assert hasattr(l, s) and s in _lib.PROTOTYPES
    assert ctypes.sizeof(A.LrRopeScaling) == 32
    assert ctypes.sizeof(A.LrLlamaArch) == 32   # unchanged
    # the header declares what _abi.py declares: same field names, in order, with the same C types
    text = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    m = re.search(r"typedef struct LrRopeScaling \{(.*?)\} LrRopeScaling;", text, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[(\d+)\]$", nm)
            base = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}[ctype]
            fields.append((arr.group(1), base * int(arr.group(2))) if arr else (nm, base))
    assert [(n, t) for n, t in fields] == [(n, t) for n, t in A.LrRopeScaling._fields_]
    assert re.search(r"int lr_llama_set_rope_scaling\(lr_llama_t\* h, const LrRopeScaling\* s\);", text)
    assert re.search(r"int lr_rope_table_ex\(float\* cs, int32_t max_positions, int32_t head_dim, float theta, "
                     r"const LrRopeScaling\* s,\s+void\* hip_stream\);", text)
    # bad arguments are refused before any device call
    L = _lib.lib()
    assert L.lr_llama_set_rope_scaling(None, None) == -1 and b"null handle" in L.lr_last_error()
    assert L.lr_rope_table_ex(None, 8, 64, 1e4, None, None) == -1


def _kernels(asm_text):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, flags=re.M)
    out = {}
    for n in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*s_endpgm" % re.escape(n), asm_text, flags=re.M | re.S)
        assert m, n
        out[n] = [ln.split(";")[0].strip() for ln in m.group(1).splitlines()
                  if ln.split(";")[0].strip() and not ln.strip().startswith(".") and not ln.strip().endswith(":")]
    return out


def test_hd64_attention_isa_keeps_m0_vmcnt_no_scratch_and_its_register_budget(tmp_path):
    """llama_attn_hd64.hip issues LDS-DMA from inline asm like variants 2 and 4 (tests/test_isa_checks.py explains why): every
    M0 write is the asm block's own and serves the DMA right behind it, an `s_waitcnt vmcnt` stands between every barrier and
    the DMAs before it, there is one product kernel, it spills nothing and uses no scratch, and its register count keeps
    three workgroups on a CU."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function"]
    out = tmp_path / "hd64.s"
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "llama_attn_hd64.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    kernels = _kernels(text)
    assert len(kernels) == 1 and "attn_hd64_kernel" in next(iter(kernels)), list(kernels)   # the product kernel
    body = next(iter(kernels.values()))
    dma = re.compile(r"^(global_load_lds_\w+|buffer_load_\w+ .*\blds\b)")
    dma_at = [i for i, ln in enumerate(body) if dma.match(ln)]
    assert len(dma_at) >= 4
    for i, ln in enumerate(body):
        assert not re.match(r"^(s_movrel\w*|v_movrel\w*|s_set_gpr_idx\w*|ds_gws_\w+|s_sendmsg\w*)\b", ln), ln
        if re.search(r"\bm0\b", ln):
            assert re.match(r"s_mov_b32 m0, s\d+$", ln), ln
            assert any(dma.match(x) for x in body[i + 1:i + 4]), (ln, body[i + 1:i + 4])
    for i in dma_at:
        assert any(re.match(r"s_mov_b32 m0, s\d+$", x) for x in body[max(0, i - 3):i]), body[i]
    barriers = 0
    for i, ln in enumerate(body):
        if ln.startswith("s_barrier"):
            barriers += 1
            for x in reversed(body[:i]):
                if re.match(r"s_waitcnt .*vmcnt\(\d+\)", x):
                    break
                assert not dma.match(x), "LDS-DMA reaches a barrier without a vmcnt wait"
    assert barriers >= 2
    assert not any(ln.startswith("scratch_") or ln.startswith("buffer_store") for ln in body)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", text) and re.search(r"\.vgpr_spill_count:\s+0\b", text)
    assert re.search(r"\.sgpr_spill_count:\s+0\b", text)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", text)
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1))
    agprs = int(re.search(r"\.agpr_count:\s+(\d+)", text).group(1))
    assert 0 < vgprs + agprs <= HD64_VGPR_BOUND, (vgprs, agprs)
    assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text).group(1)) <= HD64_VGPR_BOUND
    # the steady state's MFMAs: 16 for S^T, 16 + 2 for O^T and the row sums, per key block and stage buffer
    assert sum(ln.startswith("v_mfma_f32_16x16x32_bf16") for ln in body) == 2 * 36
    assert sum(ln.startswith("ds_read_b64_tr_b16") for ln in body) == 2 * 16
