"""GPU: the Gemma ranker -- attention variant 4 (head_dim-256 MFMA flash attention), the GeGLU epilogue, the Gemma RMSNorm
in the fused split-K reduce, and the whole scoring path against the reference's goldens and the torch restatement."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llamarec_amd.synth import bf16_round, hash_uniform, synth_gemma_state
from tests.test_gemma_host import load_gemma_golden
from tests.test_gpu_llama import attention, attention_ref, dev_bf16, host_f32

LENS = [1, 63, 64, 65, 128, 129, 300, 2, 256, 257, 600, 1125]


@pytest.mark.parametrize("nh,nkv", [(8, 1), (4, 4), (16, 16), (8, 2)])
def test_hd256_attention_vs_numpy(nh, nkv):
    cu = np.concatenate([[0], np.cumsum(LENS)])
    qkv = bf16_round(hash_uniform(nh * 100 + nkv, (cu[-1], (nh + 2 * nkv) * 256), 1.0))
    got = attention(qkv, cu, nh, nkv, 256, 4)
    ref = attention_ref(qkv, cu, nh, nkv, 256)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    assert err.max() < 1.5e-2, err.max()
    gen = attention(qkv, cu, nh, nkv, 256, 1)             # the generic kernel at the same rounding points
    assert np.abs(gen - ref).max() < 1.5e-2


def test_hd256_attention_refuses_other_head_dims():
    from llamarec_amd._lib import lib, stream_ptr

    qkv = torch.zeros((10, 3 * 128), dtype=torch.int16, device="cuda")
    out = torch.zeros((10, 128), dtype=torch.int16, device="cuda")
    cu = np.array([0, 10], np.int32)
    cud = torch.from_numpy(cu).cuda()
    rc = lib().lr_attention_varlen(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, 1, 1, 1, 128, 4,
                                   stream_ptr())
    assert rc == -2 and b"head_dim 256" in lib().lr_last_error()


def test_hd256_attention_rows_are_batch_invariant():
    nh, nkv = 8, 1
    rng = np.random.default_rng(1)
    lens = [700, 129, 1125, 5]
    cu = np.concatenate([[0], np.cumsum(lens)])
    qkv = bf16_round(rng.standard_normal((cu[-1], (nh + 2 * nkv) * 256)).astype(np.float32))
    full = attention(qkv, cu, nh, nkv, 256, 4)
    for b in (0, 2, 3):
        alone = attention(qkv[cu[b]:cu[b + 1]], np.array([0, lens[b]]), nh, nkv, 256, 4)
        assert np.array_equal(alone, full[cu[b]:cu[b + 1]]), b


def test_hd256_online_softmax_with_forced_maximum_jumps():
    """As test_attention_online_softmax_with_forced_maximum_jumps (tests/test_gpu_llama.py) at head_dim 256: keys far into a
    prompt copy the direction of chosen queries at large gains, so some rows' maximum jumps past the deferral threshold at
    chosen (off-diagonal, first, diagonal) blocks; a float64 reference with bf16 probabilities."""
    nh = nkv = 2
    hd = 256
    lens = [700, 333]
    cu = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(3)
    n = int(cu[-1])
    qkv = (rng.standard_normal((n, 3 * nh * hd)) * 0.3).astype(np.float32)
    q = qkv[:, : nh * hd].reshape(n, nh, hd)
    k = qkv[:, nh * hd: 2 * nh * hd].reshape(n, nh, hd)
    spikes = [(200, [450, 460, 699], 9.0), (330, [600, 601], 25.0), (70, [500], 3.0), (5, [40, 300], 12.0),
              (640, [650, 690], 14.0), (700 + 100, [700 + 250, 700 + 332], 20.0)]
    for key, qs, gain in spikes:
        for h in range(nh):
            k[key, h] = gain * np.mean([q[j, h] for j in qs], axis=0)
    qkv = bf16_round(qkv)
    got = attention(qkv, cu, nh, nkv, hd, 4)
    qq = qkv[:, : nh * hd].reshape(n, nh, hd).astype(np.float64)
    kk = qkv[:, nh * hd: 2 * nh * hd].reshape(n, nh, hd).astype(np.float64)
    vv = qkv[:, 2 * nh * hd:].reshape(n, nh, hd).astype(np.float64)
    ref = np.zeros((n, nh * hd))
    jumps = 0
    for b in range(len(lens)):
        s, e = cu[b], cu[b + 1]
        T = e - s
        mask = np.tril(np.ones((T, T), bool))
        for h in range(nh):
            sc = np.where(mask, (qq[s:e, h] @ kk[s:e, h].T) / np.sqrt(hd), -np.inf)
            for blk in range(1, (T + 63) // 64):   # a later block's maximum past everything before it by > 2^8
                before = sc[:, : blk * 64].max(-1)
                here = sc[:, blk * 64: (blk + 1) * 64].max(-1)
                jumps += int((((here - before) * 1.4426950408889634) > 8.0).sum())
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[s:e, h * hd:(h + 1) * hd] = (p @ vv[s:e, h]) / p.sum(-1, keepdims=True)
    assert jumps > 10
    assert np.isfinite(got).all()
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() < 2.0e-2 * max(1.0, scale), (np.abs(got - ref).max(), scale)


def _gated(epi, M, N, K, variant, A, B, ws=None):
    from llamarec_amd._lib import check, lib, stream_ptr

    Cm = torch.full((M, N // 2), float("nan"), dtype=torch.bfloat16, device="cuda")
    check(lib().lr_gemm_bf16_nt_epi(A.data_ptr(), B.data_ptr(), Cm.data_ptr(), None, M, N, K, epi, variant, None, None, 0,
                                    0, 0, ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                    stream_ptr()), "gemm")
    torch.cuda.synchronize()
    return Cm


@pytest.mark.parametrize("M", [1000, 517, 7])
def test_geglu_epilogue_fast_equals_generic_bit_for_bit(M):
    g = torch.Generator(device="cuda").manual_seed(M)
    K, N = 512, 1024
    A = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g, device="cuda") * 0.1).to(torch.bfloat16)
    ref = _gated(5, M, N, K, 1, A, B)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(_gated(5, M, N, K, 4, A, B).view(torch.int16), ref.view(torch.int16))
    swi = _gated(2, M, N, K, 1, A, B)
    assert not torch.equal(swi, ref)                                  # it is not SiLU
    # against torch: gelu_pytorch_tanh(bf16 gate) * bf16 up at the same rounding points (1 bf16 ulp)
    acc = (A.float() @ B.float().T).view(M, N // 32, 2, 16)
    gate, up = acc[:, :, 0].reshape(M, N // 2).bfloat16(), acc[:, :, 1].reshape(M, N // 2).bfloat16()
    want = (torch.nn.functional.gelu(gate, approximate="tanh") * up).float()
    assert ((ref.float() - want).abs() <= want.abs() * 2 ** -7 + 1e-6).float().mean() > 0.99
    # ... and every element within the strict bound of the float64 reference (test_gpu_stage2_bounds.gated_ratio)
    from tests.test_gpu_stage2_bounds import gated_ratio

    A64, B64 = A.double().cpu().numpy(), B.double().cpu().numpy()
    r = gated_ratio(5, A64 @ B64.T, np.abs(A64) @ np.abs(B64).T, K, ref.float().cpu().numpy())
    assert r <= 1.0, r
    # the split-K reduce (latency mode) with the GeGLU epilogue: exact integer partial sums -> the generic kernel's bits
    Ai = (torch.arange(M * 4096, device="cuda").view(M, 4096) % 5 - 2).to(torch.bfloat16)
    Bi = ((torch.arange(N * 4096, device="cuda").view(N, 4096) * 3) % 7 - 3).to(torch.bfloat16) * 0.0625
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    split = _gated(5, min(M, 256), N, 4096, 5, Ai[:256], Bi, ws)
    assert torch.equal(split.view(torch.int16), _gated(5, min(M, 256), N, 4096, 1, Ai[:256], Bi).view(torch.int16))


@pytest.mark.parametrize("M,N,K", [(460, 2048, 2048), (23, 2048, 16384), (300, 3072, 4096)])
def test_gemma_norm_fused_splitk_reduce_is_bit_identical(M, N, K):
    from llamarec_amd._lib import check, lib, stream_ptr

    A = bf16_round(hash_uniform(M + N, (M, K), 1.0))
    B = bf16_round(hash_uniform(K + 3, (N, K), 0.05))
    R = bf16_round(hash_uniform(11, (M, N), 2.0))
    w = bf16_round(hash_uniform(5, (N,), 0.3))
    a, b, wd = dev_bf16(A), dev_bf16(B), dev_bf16(w)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    outs = {}
    for fuse in (0, 1):
        c = dev_bf16(R).clone()
        xn = torch.full((M, N), 0x7FC0, dtype=torch.int16, device="cuda")
        was = C.c_int32(-1)
        check(lib().lr_gemm_bf16_nt_residual_rmsnorm_ex(a.data_ptr(), b.data_ptr(), c.data_ptr(), c.data_ptr(), M, N, K, 5,
                                                        wd.data_ptr(), xn.data_ptr(), 1e-6, 1, fuse, C.byref(was),
                                                        ws.data_ptr(), ws.numel(), stream_ptr()), "gemm + gemma norm")
        torch.cuda.synchronize()
        outs[fuse] = (c.cpu().numpy().copy(), xn.cpu().numpy().copy(), was.value)
    assert outs[0][2] == 0 and outs[1][2] == 1
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    got_c = host_f32(torch.from_numpy(outs[1][0]))
    rstd = 1.0 / np.sqrt((got_c.astype(np.float64) ** 2).mean(-1, keepdims=True) + 1e-6)
    xn_ref = (got_c * rstd * (1.0 + w)).astype(np.float32)           # (1 + w), fp32, one rounding
    got_xn = host_f32(torch.from_numpy(outs[1][1]))
    assert np.abs(got_xn - xn_ref).max() <= 2 ** -7 * max(1.0, np.abs(xn_ref).max())


@pytest.mark.parametrize("name", ["tiny_hd256_mqa", "tiny_hd256_wide", "tiny_hd16"])
@pytest.mark.parametrize("variants", [(0, 0), (1, 1), (4, 4), (5, 0)])
def test_gemma_prefill_vs_reference_goldens(golden_dir, name, variants):
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_gemma_golden(golden_dir, name)
    model = LlamaRanker.from_state_dict(sd, cfg)
    assert model.family == "gemma"
    if variants[1] == 4 and cfg["head_dim"] != 256:
        with pytest.raises(RuntimeError, match="head_dim 256"):
            model.set_variants(*variants).last_logits(seqs)
        return
    model.set_variants(*variants)
    got = model.last_logits(seqs).cpu().numpy()
    assert got.shape == z["logits_bf16"].shape and np.array_equal(got, bf16_round(got))
    assert np.abs(got - z["logits_bf16"]).max() < 3e-2
    assert np.abs(got - z["logits_fp32"]).max() < 3e-2
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])
    assert np.abs(scores - z["scores_bf16"]).max() < 3e-2


@pytest.mark.parametrize("name", ["tiny_hd256_mqa", "tiny_hd256_wide"])
def test_gemma_last_layer_pruning_matches_full_last_layer(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_gemma_golden(golden_dir, name)
    model = LlamaRanker.from_state_dict(sd, cfg)
    pruned = model.last_logits(seqs).cpu().numpy()
    full = model.set_last_layer_pruning(False).last_logits(seqs).cpu().numpy()
    assert np.abs(pruned - full).max() < 2e-2
    assert np.abs(full - z["logits_bf16"]).max() < 3e-2


def test_gemma_handle_refuses_lora_and_folded_norms(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd._lib import lib
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_gemma_golden(golden_dir, "tiny_hd256_mqa")
    model = LlamaRanker.from_state_dict(sd, cfg)
    with pytest.raises(NotImplementedError, match="folded"):
        model.set_fold_norms(True)
    # ... and the library itself refuses folded matrices for a Gemma handle (the Python guard above never reaches it)
    L = cfg["num_hidden_layers"]
    w = model._tensors["0.wqkv"]
    arr = (C.c_void_p * L)(*([w.data_ptr()] * L))
    assert lib().lr_llama_set_folded_norms(model._h, arr, arr) == -2 and b"Gemma" in lib().lr_last_error()
    assert lib().lr_llama_set_folded_norms(model._h, None, None) == 0      # "no folded norms" stays valid
    lc = A.LrLoraTrainConfig(r=8, alpha=32.0, dropout=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, seed=1)
    layers = (A.LrLlamaLayerWeightsT * cfg["num_hidden_layers"])()
    wt = A.LrLlamaWeightsTDesc(layers=layers, lm_head_t=None)
    h = C.c_void_p()
    rc = lib().lr_llama_lora_create(model._h, C.byref(wt), C.byref(lc), None, 0, None, C.byref(h))
    assert rc == -2 and b"Llama base" in lib().lr_last_error()
    # the handle still scores after the refusals
    assert np.abs(model.last_logits(seqs).cpu().numpy() - z["logits_bf16"]).max() < 3e-2


def test_geglu_handle_with_llama_norm_refuses_folded_norms():
    """Arch (norm_style 0, mlp_act 1): no preset builds it, but the C ABI accepts it. A folded gate-up product needs a
    row scale, which the GeGLU epilogue does not take, so the handle must refuse folded matrices (it used to run SwiGLU)."""
    from llamarec_amd import _abi as A
    from llamarec_amd._lib import lib

    w = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    cfg = A.LrLlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=64, num_layers=1, num_heads=1, num_kv_heads=1,
                          head_dim=64, max_positions=16, rms_eps=1e-6, rope_theta=10000.0)
    layers = (A.LrLlamaLayerWeights * 1)()
    for field in ("input_norm", "wqkv", "wo", "post_norm", "wgu", "wdown"):
        setattr(layers[0], field, w.data_ptr())
    desc = A.LrLlamaWeightsDesc(embed=w.data_ptr(), final_norm=w.data_ptr(), lm_head=w.data_ptr(), layers=layers)
    arch = A.LrLlamaArch(norm_style=0, mlp_act=1, embed_scale=1.0)
    h = C.c_void_p()
    assert lib().lr_llama_create_ex(C.byref(cfg), C.byref(arch), C.byref(desc), C.byref(h)) == 0
    try:
        arr = (C.c_void_p * 1)(w.data_ptr())
        assert lib().lr_llama_set_folded_norms(h, arr, arr) == -2 and b"GeGLU" in lib().lr_last_error()
        assert lib().lr_llama_set_folded_norms(h, None, None) == 0
    finally:
        lib().lr_llama_destroy(h)


@pytest.mark.parametrize("which,lens", [("2b", [460, 1125, 700, 5]), ("7b", [600, 1000])])
def test_full_width_gemma_fast_vs_generic_and_restatement(which, lens):
    """Gemma-2B (8 x 256 MQA heads on 2048) and Gemma-7B (16 x 256 on 3072: nh * hd != hidden) layer shapes, 2 layers,
    random weights, long prompts: the fast path (256-tile GEMMs with the GeGLU and hd-256 RoPE epilogues, attention
    variant 4, pruned last layer, split-K B-row products with the fused Gemma norm) against the generic kernels, and both
    against the fp32 torch restatement on the GPU."""
    from llamarec_amd.llm import GEMMA_2B, GEMMA_7B, LlamaRanker
    from tests import gemma_ref as G

    cfg = dict(GEMMA_2B if which == "2b" else GEMMA_7B, num_hidden_layers=2, vocab_size=32000)
    sd = G.random_gemma_state(cfg, seed=7, device="cuda")
    model = LlamaRanker.from_state_dict(sd, cfg)
    rng = np.random.default_rng(2)
    seqs = [np.concatenate([[2], rng.integers(3, 32000, size=n - 1)]).astype(np.int32) for n in lens]
    label_ids = list(range(100, 120))
    fast = model.prefill_verbalize(seqs, label_ids).cpu().numpy()
    gen = model.set_variants(1, 1).prefill_verbalize(seqs, label_ids).cpu().numpy()
    lat = model.set_variants(5, 0).prefill_verbalize(seqs[:1], label_ids).cpu().numpy()
    model.set_variants(0, 0)
    ref = G.last_logits(sd, cfg, seqs, torch.float32, device="cuda")[:, label_ids]
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"gemma-{which}: max |ref| {np.abs(ref).max():.3f}, fast-ref {np.abs(fast - ref).max():.4f}, "
          f"gen-ref {np.abs(gen - ref).max():.4f}, fast-gen {np.abs(fast - gen).max():.4f}")
    assert np.isfinite(fast).all() and float(np.abs(fast).max()) > 0.05
    assert np.abs(fast - gen).max() <= 5e-2 * scale
    assert np.abs(fast - ref).max() <= 1e-1 * scale and np.abs(gen - ref).max() <= 1e-1 * scale
    assert np.abs(lat - fast[:1]).max() <= 5e-2 * scale
    # a prompt's scores do not depend on the rest of the batch
    alone = model.prefill_verbalize([seqs[1]], label_ids).cpu().numpy()
    assert np.array_equal(alone[0], fast[1])


def test_gemma_online_single_user_path_and_pipeline():
    """demo/inference.py's flow and the two-stage pipeline with a Gemma ranker, unchanged callers."""
    from llamarec_amd import data as D
    from llamarec_amd import inference as I
    from llamarec_amd.llm import LlamaRanker, pack_prompts
    from llamarec_amd.lru import LRURec, init_lru_state_dict
    from llamarec_amd.pipeline import TwoStagePipeline
    from llamarec_amd.verb import ManualVerbalizer
    from tests import gemma_ref as G
    from tests.fake_tokenizer import FakeTokenizer

    ds = D.synthetic_dataset(num_users=5, num_items=400, seed=3)
    retr = LRURec.from_state_dict(init_lru_state_dict(400, seed=9))
    query = ds["train"][1][-7:]
    cands = I.retrieve_candidates(retr, query, top_k=20)
    prompt = I.generate_prompt(query, cands, ds["meta"])
    tok = FakeTokenizer()
    cfg = dict(model_type="gemma", vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
               num_attention_heads=2, num_key_value_heads=1, head_dim=256, max_position_embeddings=2048,
               rms_norm_eps=1e-6, rope_theta=10000.0)
    gsd = synth_gemma_state(cfg, 11)
    ranker = LlamaRanker.from_state_dict(gsd, cfg)
    verb = ManualVerbalizer(tokenizer=tok, classes=list(range(20)), label_words={i: chr(65 + i) for i in range(20)})
    top = I.rank_candidates(ranker, tok, prompt, cands, verb, top_k=10)
    assert len(top) == 10 and set(top) <= set(cands)
    ids = np.asarray(tok(prompt)["input_ids"])
    ref = G.last_logits(gsd, cfg, [ids], torch.bfloat16)[0][verb.label_token_ids]
    got = ranker.prefill_verbalize([ids], verb.label_token_ids)[0].cpu().numpy()
    assert np.abs(got - ref).max() < 3e-2
    # two-stage pipeline step with the Gemma ranker
    rng = np.random.default_rng(0)
    B, L = 4, 30
    hist = np.zeros((B, L), np.int64)
    for b in range(B):
        n = int(rng.integers(1, L + 1))
        hist[b, L - n:] = rng.choice(400, size=n, replace=False) + 1
    labels = rng.integers(1, 401, size=B)
    seqs = [np.concatenate([[2], rng.integers(3, 1024, size=int(n))]) for n in rng.integers(4, 150, size=B)]
    pipe = TwoStagePipeline(retr, ranker, list(range(40, 60)), device="cuda:0")
    pids, cu = pack_prompts(seqs)
    pipe.step(torch.from_numpy(hist).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(pids).cuda(),
              torch.from_numpy(cu).cuda(), cu)
    _, _, n = pipe.finish()
    torch.cuda.synchronize()
    assert n == B
    scores = ranker.prefill_verbalize(seqs, list(range(40, 60))).cpu().numpy()
    ref = G.last_logits(gsd, cfg, seqs, torch.bfloat16)[:, 40:60]
    assert np.abs(scores - ref).max() < 3e-2


def _write_gemma_hf_dir(path, sd, cfg):
    """A local Gemma checkpoint directory as the reference's from_pretrained reads it: config.json with model_type gemma
    and one safetensors file of bf16 tensors under HF's names (no lm_head: tied to the embedding)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    json.dump(dict(cfg, architectures=["GemmaForCausalLM"], torch_dtype="bfloat16"), open(os.path.join(path, "config.json"), "w"))
    save_file({n: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for n, v in sd.items()},
              os.path.join(path, "model.safetensors"), metadata={"format": "pt"})


def test_gemma_from_pretrained_with_default_args_is_nf4_like_the_reference(golden_dir, tmp_path):
    """`train_ranker.py --llm gemma --eval_only --llm_base_model <dir>` loads with the parsed defaults, which include
    --llm_load_in_4bit (the reference quantises Gemma's Linears through the same BitsAndBytesConfig, train_ranker.py:49-59):
    the local directory loads, every Linear goes through the NF4 round trip (embedding / tied lm_head and norms do not),
    and the scores equal the restatement run on the round-tripped weights."""
    from llamarec_amd import config as cfgmod
    from llamarec_amd._lib import check, lib, stream_ptr
    from llamarec_amd.llm import LlamaRanker
    from tests import gemma_ref as G

    args = cfgmod.parse(["--dataset_code", "beauty", "--llm", "gemma", "--eval_only"], model_code="llm")
    assert args.llm_load_in_4bit is True
    z, cfg, sd, seqs = load_gemma_golden(golden_dir, "tiny_hd256_mqa")
    hf = str(tmp_path / "gemma")
    _write_gemma_hf_dir(hf, sd, cfg)
    loaded = LlamaRanker.from_pretrained(hf, load_in_4bit=args.llm_load_in_4bit)
    assert loaded.family == "gemma" and loaded.hd == 256
    label_ids = list(z["label_ids"])
    got = loaded.prefill_verbalize(seqs, label_ids)
    direct = LlamaRanker.from_state_dict(sd, cfg, nf4=True).prefill_verbalize(seqs, label_ids)
    plain = LlamaRanker.from_state_dict(sd, cfg, nf4=False).prefill_verbalize(seqs, label_ids)
    assert torch.isfinite(got).all() and torch.equal(got, direct)
    assert not torch.equal(got, plain)                                       # the round trip really ran
    # restatement on the round-tripped Linears
    nsd = {}
    scratch = None
    for name, v in sd.items():
        t = torch.from_numpy(v).cuda().to(torch.bfloat16).contiguous()
        if name.endswith("_proj.weight"):
            need = lib().lr_nf4_scratch_bytes(t.numel())
            scratch = torch.empty(need, dtype=torch.uint8, device="cuda") if scratch is None or scratch.numel() < need else scratch
            check(lib().lr_nf4_roundtrip_bf16(t.data_ptr(), t.numel(), 1, t.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                              stream_ptr()), "nf4")
        nsd[name] = t.float()
    torch.cuda.synchronize()
    ref = G.last_logits(nsd, cfg, seqs, torch.bfloat16, device="cuda")[:, label_ids]
    assert np.abs(got.cpu().numpy() - ref).max() < 3e-2


def test_train_ranker_gemma_eval_only_end_to_end(tmp_path):
    """`train_ranker.py --llm gemma --eval_only` with default flags (NF4 on) scores the retrieved users through the Gemma
    ranker and writes the reference's metric files; training a Gemma base is refused."""
    import pickle

    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    r = pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))
    if not r["test_users"]:
        pytest.skip("random retriever retrieved nobody")
    out = str(tmp_path / "experiments" / "gemma" / "synthetic")
    metrics, overall = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma", "--eval_only",
                                          "--llm_retrieved_path", lru_root, "--export_root", out, "--llm_max_history", "5"])
    assert "test_NDCG@10" in metrics and 0.0 <= metrics["test_NDCG@10"] <= 1.0
    assert os.path.exists(os.path.join(out, "subset_metrics.json")) and os.path.exists(os.path.join(out, "overall_metrics.json"))
    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma", "--llm_retrieved_path", lru_root,
                           "--export_root", out])

