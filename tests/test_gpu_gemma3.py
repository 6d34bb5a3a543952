"""GPU: the Gemma-3 ranker (model_type "gemma3_text", lr_llama_set_gemma3) against the committed goldens of
tests/gen_goldens_gemma3.py: sliding-window layers (the windowed head_dim-256 MFMA kernels, the generic kernel at head_dim
128), two rotary tables picked per layer, the q/k norm in Gemma's rounding, sandwich norms. Every archive within its own
tolerance on every route, and more than ten tolerances from every mutant of the restatement: that part fails on a tree without
the family (model_type "gemma3_text" is refused there), and on one that drops the window, the local rotary base or the (1 + w)
norm."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import gemma3_ref as G3
from tests.gen_goldens_gemma3 import WEAK_MUTANTS, golden_tolerance
from tests.test_gemma3_host import GEMMA3_GOLDENS, load_gemma3_golden

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
_MODELS = {}


def _lib():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def _golden_model(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker

    if name not in _MODELS:
        z, cfg, sd, seqs = load_gemma3_golden(golden_dir, name)
        _MODELS[name] = (z, cfg, sd, [np.asarray(s, np.int32) for s in seqs], LlamaRanker.from_state_dict(sd, cfg))
    return _MODELS[name]


@pytest.mark.parametrize("name", GEMMA3_GOLDENS)
def test_gemma3_goldens_on_every_route_and_far_from_every_mutant(golden_dir, name):
    z, cfg, sd, seqs, model = _golden_model(golden_dir, name)
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    assert model.family == "gemma3" and model.max_prompt_len is None and max(map(len, seqs)) > cfg["sliding_window"]
    routes = {}
    for label, (gemm, attn, prune) in {"default": (6, 0, True), "generic attention": (6, 1, True), "unpruned": (6, 0, False),
                                       "generic, unpruned": (1, 1, False), "variant 4": (0, 4, True)}.items():
        if attn == 4 and cfg["head_dim"] != 256:
            continue
        got = model.set_variants(gemm, attn).set_last_layer_pruning(prune).last_logits(seqs).cpu().numpy()
        routes[label] = got
        print(f"gemma3 {name} {label}: tol {tol:.4f}, vs bf16 {np.abs(got - z['logits_bf16']).max():.4f}, "
              f"vs fp32 {np.abs(got - z['logits_fp32']).max():.4f}")
        assert np.isfinite(got).all()
        assert np.abs(got - z["logits_bf16"]).max() < tol, label
        assert np.abs(got - z["logits_fp32"]).max() < tol, label
    model.set_variants(6, 0).set_last_layer_pruning(True)
    assert np.abs(routes["default"] - routes["unpruned"]).max() < tol
    got = routes["default"]
    for m in G3.MODEL_MUTANTS:
        d = float(np.abs(got - z[f"mutant_{m}"]).max())
        print(f"gemma3 {name}: {d / tol:.1f} tolerances from mutant {m}")
        if m in WEAK_MUTANTS.get(name, ()):
            continue
        assert d > 10 * tol, (m, d, tol)
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])
    alone = model.last_logits([seqs[-2]]).cpu().numpy()            # a prompt's logits do not depend on the batch
    assert np.array_equal(alone[0], got[-2])


@pytest.mark.parametrize("name", ["tiny_hd256_mqa", "tiny_hd128"])
def test_shared_prefix_within_the_window_is_bit_identical_and_beyond_it_runs_whole(golden_dir, name):
    from llamarec_amd.llm import common_prefix_len, pack_prompts

    z, cfg, sd, seqs, model = _golden_model(golden_dir, name)
    W, V = cfg["sliding_window"], cfg["vocab_size"]
    label_ids = list(z["label_ids"])
    rng = np.random.default_rng(W)

    def prompts(P, tails):
        head = np.concatenate([[2], rng.integers(3, V, size=P - 1)])
        return [np.concatenate([head, [3 + b], rng.integers(3, V, size=n)]).astype(np.int32) for b, n in enumerate(tails)]

    P = W // 2
    for tails, within in (([0, 3, W - P - 2, 1], True), ([0, 3, 2 * W, 70], False)):
        ps = prompts(P, tails)
        assert common_prefix_len(*pack_prompts(ps)) == P and (max(map(len, ps)) <= W) == within
        for prune in (True, False):
            model.set_last_layer_pruning(prune)
            shared = model.prefill_verbalize(ps, label_ids, share_prefix=True)
            plain = model.prefill_verbalize(ps, label_ids, share_prefix=False)
            assert torch.isfinite(shared).all() and torch.equal(shared, plain), (within, prune)
        model.set_last_layer_pruning(True)
        # the answer is the restatement's: with a long prompt in the batch, also for the short prompts beside it
        ref = G3.last_logits(sd, cfg, ps, torch.bfloat16)[:, label_ids]
        r32 = G3.last_logits(sd, cfg, ps, torch.float32)[:, label_ids]
        tol = golden_tolerance(r32, ref)
        assert np.abs(plain.cpu().numpy() - ref).max() < tol and np.abs(plain.cpu().numpy() - r32).max() < tol


def test_set_gemma3_refusals_leave_the_handle_scoring_and_null_restores_gemma_v1(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.synth import synth_llama_state

    L, _ = _lib()
    z, cfg, sd, seqs, model = _golden_model(golden_dir, "tiny_hd256_mqa")
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    nl = cfg["num_hidden_layers"]
    before = model.last_logits(seqs)
    good, arrs = model.gemma3_ext()

    def ext(**kw):
        e = A.LrGemma3Ext(sliding_window=good.sliding_window, rope_theta_local=good.rope_theta_local,
                          global_linear_factor=good.global_linear_factor, attn_scale=good.attn_scale, layer_is_sliding=arrs[0])
        e.q_norm, e.k_norm, e.attn_out_norm, e.mlp_out_norm = arrs[1:]
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    first = arrs[1][0]
    null_layer = (C.c_void_p * nl)(*([first] + [None] * (nl - 1)))
    misaligned = (C.c_void_p * nl)(*([first + 2] * nl))
    bad_kinds = (C.c_uint8 * nl)(*([2] + [0] * (nl - 1)))
    bad = [ext(sliding_window=0), ext(sliding_window=-5), ext(rope_theta_local=float("nan")), ext(rope_theta_local=-1.0),
           ext(rope_theta_local=0.0), ext(global_linear_factor=float("inf")), ext(global_linear_factor=-8.0),
           ext(attn_scale=float("nan")), ext(attn_scale=-0.5), ext(reserved=(C.c_int32 * 4)(0, 0, 1, 0)), ext(q_norm=None),
           ext(layer_is_sliding=None), ext(mlp_out_norm=None), ext(k_norm=null_layer), ext(q_norm=misaligned),
           ext(attn_out_norm=misaligned), ext(layer_is_sliding=bad_kinds)]
    for i, e in enumerate(bad):
        assert L.lr_llama_set_gemma3(model._h, C.byref(e)) == LR_EINVAL and L.lr_last_error(), i
        assert torch.equal(model.last_logits(seqs), before), i
    assert L.lr_llama_set_gemma3(None, C.byref(good)) == LR_EINVAL
    assert L.lr_llama_set_gemma3(model._h, C.byref(ext(attn_scale=0.3))) == LR_EUNSUPPORTED          # a foreign score scale
    assert L.lr_llama_set_gemma3(model._h, C.byref(ext(attn_scale=cfg["head_dim"] ** -0.5))) == 0   # the kernels' own
    assert torch.equal(model.last_logits(seqs), before)
    # the other extensions, folded norms and LoRA engines refuse such a handle
    qa = (C.c_void_p * nl)(*([first] * nl))
    assert L.lr_llama_set_qk_norm(model._h, qa, qa) == LR_EUNSUPPORTED
    assert L.lr_llama_set_qkv_bias(model._h, qa) == LR_EUNSUPPORTED
    assert L.lr_llama_set_gemma2(model._h, C.byref(A.LrGemma2Ext(attn_softcap=50.0))) == LR_EUNSUPPORTED
    assert L.lr_llama_set_gemma2(model._h, None) == 0                       # (nothing of Gemma-2's to take off)
    assert L.lr_llama_set_folded_norms(model._h, qa, qa) == LR_EUNSUPPORTED
    assert L.lr_llama_set_folded_norms(model._h, None, None) == 0
    with pytest.raises(NotImplementedError, match="folded"):
        model.set_fold_norms(True)
    lc = A.LrLoraTrainConfig(r=8, alpha=32.0, dropout=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, seed=1)
    wt = A.LrLlamaWeightsTDesc(layers=(A.LrLlamaLayerWeightsT * nl)(), lm_head_t=None)
    h = C.c_void_p()
    assert L.lr_llama_lora_create(model._h, C.byref(wt), C.byref(lc), None, 0, None, C.byref(h)) == LR_EUNSUPPORTED
    assert L.lr_llama_lora_create_ex(model._h, C.byref(wt), C.byref(lc), None, None, 0, None, C.byref(h)) == LR_EUNSUPPORTED
    assert torch.equal(model.last_logits(seqs), before)
    # handles the extension does not fit: a Llama norm, a Gemma-2 extension, Qwen3 norms
    lcfg = dict(vocab_size=320, hidden_size=256, intermediate_size=512, num_hidden_layers=nl, num_attention_heads=1,
                num_key_value_heads=1, max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0)
    llama = LlamaRanker.from_state_dict(synth_llama_state(lcfg, 5), lcfg)
    assert L.lr_llama_set_gemma3(llama._h, C.byref(good)) == LR_EUNSUPPORTED and b"Gemma norm" in L.lr_last_error()
    assert L.lr_llama_set_qk_norm(llama._h, qa, qa) == 0
    assert L.lr_llama_set_gemma3(llama._h, C.byref(good)) == LR_EUNSUPPORTED
    # NULL: Gemma v1's layer on the same weights -- the scores of a Gemma handle built from them -- and back again
    assert L.lr_llama_set_gemma3(model._h, None) == 0
    plain = model.last_logits(seqs)
    assert np.abs(plain.cpu().numpy() - z["logits_bf16"]).max() > 10 * tol
    model2 = LlamaRanker(dict(cfg, model_type="gemma"), device="cuda:0")     # a Gemma v1 handle over the SAME device tensors
    model2._tensors = {k: v for k, v in model._tensors.items() if not k.endswith(("q_norm", "k_norm", "out_norm"))}
    model2._create()
    model2.set_variants(6, 0)
    assert torch.equal(model2.last_logits(seqs), plain)
    assert L.lr_llama_set_gemma3(model._h, None) == 0                       # twice is fine
    assert L.lr_llama_set_gemma3(model._h, C.byref(good)) == 0
    assert torch.equal(model.last_logits(seqs), before)
    # the workspace of a handle with the extension holds the second rotary table
    assert L.lr_llama_workspace_bytes(model._h, 1000, 8) > L.lr_llama_workspace_bytes(model2._h, 1000, 8)


def test_gemma3_from_pretrained_with_and_without_nf4(golden_dir, tmp_path):
    from safetensors.torch import save_file

    from llamarec_amd import config as cfgmod
    from llamarec_amd.llm import LlamaRanker

    args = cfgmod.parse(["--dataset_code", "beauty", "--llm", "gemma3", "--eval_only"], model_code="llm")
    assert args.llm_load_in_4bit is True
    z, cfg, sd, seqs = load_gemma3_golden(golden_dir, "tiny_hd256_linear")
    seqs = [np.asarray(s, np.int32) for s in seqs]
    hf = str(tmp_path / "gemma3")
    os.makedirs(hf)
    json.dump(dict(cfg, architectures=["Gemma3ForCausalLM"], torch_dtype="bfloat16"), open(os.path.join(hf, "config.json"), "w"))
    save_file({n: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for n, v in sd.items()},
              os.path.join(hf, "model.safetensors"), metadata={"format": "pt"})
    loaded = LlamaRanker.from_pretrained(hf, load_in_4bit=args.llm_load_in_4bit)
    assert loaded.family == "gemma3" and loaded.hd == 256 and loaded.gemma3["factor"] == 8.0
    label_ids = list(z["label_ids"])
    got = loaded.prefill_verbalize(seqs, label_ids)
    direct = LlamaRanker.from_state_dict(sd, cfg, nf4=True).prefill_verbalize(seqs, label_ids)
    plain = LlamaRanker.from_pretrained(hf).prefill_verbalize(seqs, label_ids)
    assert torch.isfinite(got).all() and torch.equal(got, direct)
    assert not torch.equal(got, plain)                                       # the round trip really ran
    assert np.abs(plain.cpu().numpy() - z["scores_bf16"]).max() < golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    for i in range(cfg["num_hidden_layers"]):       # name mapping; the norms stay out of the round trip
        p = f"model.layers.{i}."
        assert torch.equal(loaded._tensors[f"{i}.post_norm"].float().cpu(), torch.from_numpy(sd[p + "pre_feedforward_layernorm.weight"]))
        assert torch.equal(loaded._tensors[f"{i}.attn_out_norm"].float().cpu(), torch.from_numpy(sd[p + "post_attention_layernorm.weight"]))
        w = sd[p + "self_attn.q_norm.weight"]
        assert torch.equal(loaded._tensors[f"{i}.q_norm"].float().cpu()[0::2], torch.from_numpy(w[:128]))
        assert torch.equal(loaded._tensors[f"{i}.q_norm"].float().cpu()[1::2], torch.from_numpy(w[128:]))
    # the same checkpoint in transformers 5's spelling of the rotary numbers scores the same bits
    from tests.test_gemma3_host import v5

    json.dump(dict(v5(cfg, 8.0), architectures=["Gemma3ForCausalLM"]), open(os.path.join(hf, "config.json"), "w"))
    assert torch.equal(LlamaRanker.from_pretrained(hf).prefill_verbalize(seqs, label_ids), plain)
    bad = {k: v for k, v in sd.items() if k != "model.layers.1.self_attn.k_norm.weight"}
    with pytest.raises(KeyError, match="k_norm"):
        LlamaRanker.from_state_dict(bad, cfg)


def test_train_ranker_gemma3_eval_only_end_to_end(tmp_path):
    """`train_ranker.py --llm gemma3 --eval_only` with default flags (NF4 on) scores the retrieved users through a tiny Gemma-3
    ranker whose window (64) is far below its prompts' length, and writes the metric files; training is refused."""
    import pickle

    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    r = pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))
    assert r["test_users"], "the synthetic retriever retrieved nobody"
    out = str(tmp_path / "experiments" / "gemma3" / "synthetic")
    metrics, overall = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma3", "--eval_only",
                                          "--llm_retrieved_path", lru_root, "--export_root", out, "--llm_max_history", "5"])
    assert "test_NDCG@10" in metrics and 0.0 <= metrics["test_NDCG@10"] <= 1.0
    assert os.path.exists(os.path.join(out, "subset_metrics.json")) and os.path.exists(os.path.join(out, "overall_metrics.json"))
    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma3", "--llm_retrieved_path", lru_root,
                           "--export_root", out])
