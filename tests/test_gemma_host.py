"""CPU: the Gemma ranker's host side -- the torch restatement against the reference's goldens, model_type dispatch, the
--llm flag and its template, the new ABI symbol, and the build-time ISA checks of the head_dim-256 attention TU."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from llamarec_amd.synth import synth_gemma_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "llamarec_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
GEMMA_GOLDENS = ("tiny_hd256_mqa", "tiny_hd256_wide", "tiny_hd16")


def load_gemma_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"gemma_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_gemma_state(cfg, int(z["weight_seed"]))
    T = z["input_ids"].shape[1]
    seqs = [z["input_ids"][b, T - n:] for b, n in enumerate(z["lens"])]
    return z, cfg, sd, seqs


@pytest.mark.parametrize("name", GEMMA_GOLDENS)
def test_gemma_restatement_matches_reference_goldens(golden_dir, name):
    from tests import gemma_ref as G

    z, cfg, sd, seqs = load_gemma_golden(golden_dir, name)
    assert cfg["model_type"] == "gemma" and cfg["head_dim"] in (16, 256)
    l32 = G.last_logits(sd, cfg, seqs)
    assert np.abs(l32 - z["logits_fp32"]).max() < 1e-4
    assert np.abs(l32 - z["logits_fp32_unpadded"]).max() < 1e-4
    lbf = G.last_logits(sd, cfg, seqs, torch.bfloat16)
    assert np.abs(lbf - z["logits_bf16"]).max() < 2e-2
    assert np.array_equal(z["scores_bf16"], z["logits_bf16"][:, z["label_ids"]])
    # the goldens really are Gemma's arithmetic: the same weights through Llama's forms score differently
    sd_llama = dict(sd)
    for k in sd_llama:
        if k.endswith("norm.weight") or k.endswith("layernorm.weight"):
            sd_llama[k] = sd[k] + 1.0
    assert np.abs(G.last_logits(sd_llama, cfg, seqs) - l32).max() > 1e-2


def test_golden_archives_are_written_reproducibly(tmp_path):
    from tests.gen_goldens_gemma import save_npz_fixed

    arrays = dict(a=np.arange(10, dtype=np.float32), config=np.array(json.dumps({"x": 1})))
    save_npz_fixed(tmp_path / "one.npz", **arrays)
    save_npz_fixed(tmp_path / "two.npz", **arrays)
    assert (tmp_path / "one.npz").read_bytes() == (tmp_path / "two.npz").read_bytes()
    z = np.load(tmp_path / "one.npz")
    assert np.array_equal(z["a"], arrays["a"]) and json.loads(str(z["config"])) == {"x": 1}


def test_model_type_dispatch():
    from llamarec_amd.llm import GEMMA_2B, LLAMA2_7B, LlamaRanker, model_family

    assert model_family(dict(LLAMA2_7B)) == "llama"                    # no model_type: every existing config
    assert model_family(dict(LLAMA2_7B, model_type="llama", rope_scaling=None)) == "llama"
    assert model_family(dict(LLAMA2_7B, model_type="mistral", sliding_window=4096)) == "llama"
    assert model_family(GEMMA_2B) == "gemma"
    for mt in ("qwen2", "phi3", "gemma2", "bert"):
        with pytest.raises(NotImplementedError, match=mt):
            model_family(dict(LLAMA2_7B, model_type=mt))
        with pytest.raises(NotImplementedError, match="supported families"):
            LlamaRanker(dict(LLAMA2_7B, model_type=mt), device="cpu")
    with pytest.raises(NotImplementedError, match="rope_scaling"):
        model_family(dict(LLAMA2_7B, model_type="llama", rope_scaling={"rope_type": "llama3", "factor": 8.0}))
    r = LlamaRanker(dict(GEMMA_2B), device="cpu")
    assert r.family == "gemma" and r.hd == 256
    assert LlamaRanker(dict(GEMMA_2B, hidden_size=3072, num_attention_heads=16), device="cpu").hd == 256   # gemma-7b
    m = LlamaRanker(dict(LLAMA2_7B, model_type="mistral", sliding_window=100), device="cpu")
    with pytest.raises(NotImplementedError, match="sliding window"):
        m._check_lengths(np.array([0, 50, 151], np.int32))
    m._check_lengths(np.array([0, 100], np.int32))


def test_gemma_arch_words():
    from llamarec_amd.llm import GEMMA_2B, GEMMA_7B, LLAMA2_7B, LlamaRanker

    a = LlamaRanker(dict(GEMMA_2B), device="cpu").arch()
    assert (a.norm_style, a.mlp_act, a.embed_scale, list(a.reserved)) == (1, 1, 45.25, [0] * 5)   # bf16(sqrt(2048))
    assert LlamaRanker(dict(GEMMA_7B), device="cpu").arch().embed_scale == 55.5                     # bf16(sqrt(3072))
    b = LlamaRanker(dict(LLAMA2_7B), device="cpu").arch()
    assert (b.norm_style, b.mlp_act, b.embed_scale) == (0, 0, 1.0)


def test_llm_flag_and_template():
    from llamarec_amd import config as cfg

    a = cfg.parse(["--dataset_code", "beauty", "--llm", "gemma"], model_code="llm")
    assert a.llm == "gemma" and a.llm_base_model == "google/gemma-2b" and a.llm_base_tokenizer == "google/gemma-2b"
    # config.py:90-102 of the reference: gemma quarters the batches, llama3 halves them
    assert (a.lora_micro_batch_size, a.test_batch_size, a.train_batch_size) == (2, 4, 4)
    a = cfg.parse(["--dataset_code", "ml-100k", "--llm", "llama3"], model_code="llm")
    assert a.llm_base_model == "meta-llama/Meta-Llama-3-8B" and (a.lora_micro_batch_size, a.test_batch_size) == (8, 16)
    a = cfg.parse(["--dataset_code", "ml-100k"], model_code="llm")
    assert a.llm is None and a.llm_base_model == "meta-llama/Llama-2-7b-hf" and a.test_batch_size == 32
    a = cfg.parse(["--dataset_code", "beauty", "--llm", "gemma", "--llm_base_model", "/models/gemma-2b"], model_code="llm")
    assert a.llm_base_model == "/models/gemma-2b" and a.llm_base_tokenizer == "google/gemma-2b"
    for name in ("llama2", "phi3", "mistral", "gemma2", "qwen2"):
        assert cfg.parse(["--dataset_code", "beauty", "--llm", name], model_code="llm").llm == name
    with pytest.raises(SystemExit):
        cfg.build_parser().parse_args(["--llm", "gpt2"])


def test_train_ranker_refuses_to_train_a_gemma_base(tmp_path):
    import train_ranker

    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma", "--llm_retrieved_path",
                           str(tmp_path)])


def test_create_ex_is_exported():
    from llamarec_amd import _abi as A
    from llamarec_amd import _lib

    l = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("lr_llama_create_ex", "lr_gemm_bf16_nt_residual_rmsnorm_ex"):
        assert hasattr(l, s) and s in _lib.PROTOTYPES
    assert ctypes.sizeof(A.LrLlamaArch) == 32
    # a bad arch word is refused before any device call
    L = _lib.lib()
    cfg = A.LrLlamaConfig(vocab_size=8, hidden_size=64, intermediate_size=64, num_layers=1, num_heads=1, num_kv_heads=1,
                          head_dim=64, max_positions=8, rms_eps=1e-6, rope_theta=1e4)
    layers = (A.LrLlamaLayerWeights * 1)()
    desc = A.LrLlamaWeightsDesc(embed=None, final_norm=None, lm_head=None, layers=layers)
    h = ctypes.c_void_p()
    arch = A.LrLlamaArch(norm_style=2, mlp_act=0, embed_scale=1.0)
    assert L.lr_llama_create_ex(ctypes.byref(cfg), ctypes.byref(arch), ctypes.byref(desc), ctypes.byref(h)) != 0
    assert b"norm_style" in L.lr_last_error()


def _kernels(asm_text):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, flags=re.M)
    out = {}
    for n in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*s_endpgm" % re.escape(n), asm_text, flags=re.M | re.S)
        assert m, n
        out[n] = [ln.split(";")[0].strip() for ln in m.group(1).splitlines()
                  if ln.split(";")[0].strip() and not ln.strip().startswith(".") and not ln.strip().endswith(":")]
    return out


def test_hd256_attention_isa_keeps_m0_vmcnt_and_no_scratch(tmp_path):
    """llama_attn_hd256.hip issues LDS-DMA from inline asm like variant 2 (tests/test_isa_checks.py explains why): every M0
    write is the asm block's own and serves the DMA right behind it, an `s_waitcnt vmcnt` stands between every barrier and
    the DMAs before it, and the kernel spills nothing (a spill would go through scratch)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function"]
    out = tmp_path / "hd256.s"
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "llama_attn_hd256.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    kernels = _kernels(text)
    assert len(kernels) == 1 and "attn_hd256_kernel" in next(iter(kernels)), list(kernels)   # the product instantiation
    body = next(iter(kernels.values()))
    dma = re.compile(r"^(global_load_lds_\w+|buffer_load_\w+ .*\blds\b)")
    dma_at = [i for i, ln in enumerate(body) if dma.match(ln)]
    assert len(dma_at) >= 8
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
