"""CPU: the Gemma-3 ranker's host side -- model_type dispatch and its complete-config rule in both spellings of the rotary
numbers, every refusal, the two ordering pins, the preset, parameter shapes, the training refusal -- and the float64 references
of tests/gemma3_ref.py: against a dense masked softmax at tiny sizes, and the conditions on the TEST DATA that the GPU tests
rely on, checked here from the reference alone: the kernel batches meet every hazard of the windowed block walk, every mutant
of the reference is outside the bound on them, and every mutant of the model is ten tolerances away in every archive."""
import ctypes
import json
import os

import numpy as np
import pytest

from llamarec_amd.synth import bf16_round, gemma3_param_shapes, hash_uniform
from tests import gemma3_ref as G3
from tests.gen_goldens_gemma3 import GEMMA3_CONFIGS, WEAK_MUTANTS, gemma3_cfg_dict, golden_state, golden_tolerance

GEMMA3_GOLDENS = tuple(GEMMA3_CONFIGS)


def load_gemma3_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"gemma3_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    cu = np.concatenate([[0], np.cumsum(z["lens"])])
    seqs = [z["input_ids"][cu[b]:cu[b + 1]] for b in range(len(z["lens"]))]
    return z, cfg, golden_state(name, int(z["weight_seed"])), seqs


def v5(cfg, factor=None):
    """The same config in transformers 5's spelling: the four rotary numbers under rope_parameters[layer kind]."""
    out = {k: v for k, v in cfg.items() if k not in ("rope_theta", "rope_local_base_freq", "rope_scaling")}
    g = {"rope_type": "default", "rope_theta": cfg["rope_theta"]}
    if factor:
        g = {"rope_type": "linear", "factor": factor, "rope_theta": cfg["rope_theta"]}
    out["rope_parameters"] = {"full_attention": g, "sliding_attention": {"rope_type": "default",
                                                                         "rope_theta": cfg["rope_local_base_freq"]}}
    return out


def test_gemma3_model_type_dispatch_needs_a_complete_config():
    from llamarec_amd.llm import GEMMA3_1B, GEMMA3_REQUIRED_KEYS, LlamaRanker, gemma3_parameters, model_family

    assert model_family(GEMMA3_1B) == "gemma3"
    g = gemma3_parameters(GEMMA3_1B)
    assert (g["window"], g["theta_global"], g["theta_local"], g["factor"]) == (512, 1e6, 1e4, None)
    assert g["sliding"] == [(i + 1) % 6 != 0 for i in range(26)] and sum(g["sliding"]) == 22
    # layer_types wins over the pattern; either one alone is enough
    lt = ["full_attention" if i in (0, 3) else "sliding_attention" for i in range(26)]
    assert gemma3_parameters(dict(GEMMA3_1B, layer_types=lt))["sliding"] == [i not in (0, 3) for i in range(26)]
    no_pat = {k: v for k, v in GEMMA3_1B.items() if k != "sliding_window_pattern"}
    assert gemma3_parameters(dict(no_pat, layer_types=lt))["sliding"] == [i not in (0, 3) for i in range(26)]
    with pytest.raises(NotImplementedError, match=r"layer_types / sliding_window_pattern.*supported families: .*gemma2$"):
        model_family(no_pat)
    # the larger text models: linear scaling of the global layers, in both spellings
    assert gemma3_parameters(dict(GEMMA3_1B, rope_scaling={"rope_type": "linear", "factor": 8.0}))["factor"] == 8.0
    assert gemma3_parameters(v5(GEMMA3_1B)) == g
    assert gemma3_parameters(v5(GEMMA3_1B, 8.0)) == dict(g, factor=8.0)
    assert model_family(v5(GEMMA3_1B, 8.0)) == "gemma3"
    for key in GEMMA3_REQUIRED_KEYS:
        cfg = {k: v for k, v in GEMMA3_1B.items() if k != key}
        with pytest.raises(NotImplementedError, match=rf"'gemma3_text'.*{key}.*supported families: .*gemma2$"):
            model_family(cfg)
        with pytest.raises(NotImplementedError, match=key):
            model_family(dict(GEMMA3_1B, **{key: None}))
        with pytest.raises(NotImplementedError, match=key):
            LlamaRanker(cfg, device="cpu")


@pytest.mark.parametrize("change, match", [
    (dict(hidden_activation="gelu"), "hidden_activation"),
    (dict(hidden_activation=None), "hidden_activation"),
    (dict(attn_logit_softcapping=50.0), "attn_logit_softcapping"),
    (dict(final_logit_softcapping=30.0), "final_logit_softcapping"),
    (dict(attention_bias=True), "attention_bias"),
    (dict(rope_scaling={"rope_type": "yarn", "factor": 8.0}), "rope scaling"),
    (dict(rope_scaling={"rope_type": "llama3", "factor": 8.0}), "rope scaling"),
    (dict(rope_scaling={"rope_type": "linear"}), "factor"),
    (dict(rope_scaling={"rope_type": "linear", "factor": -1.0}), "factor"),
    (dict(sliding_window=0), "sliding_window"),
    (dict(sliding_window=True), "sliding_window"),
    (dict(sliding_window_pattern=0), "sliding_window_pattern"),
    (dict(layer_types=["sliding_attention"] * 3), "layer_types"),
    (dict(layer_types=["chunked_attention"] * 26), "layer_types"),
    (dict(query_pre_attn_scalar=144), "query_pre_attn_scalar"),
    (dict(head_dim=96), "head_dim"),
    (dict(rope_local_base_freq=-1.0), "rotary bases"),
])
def test_gemma3_configs_the_kernels_do_not_compute_are_refused(change, match):
    from llamarec_amd.llm import GEMMA3_1B, model_family

    with pytest.raises(NotImplementedError, match=rf"{match}.*supported families: .*gemma2$"):
        model_family(dict(GEMMA3_1B, **change))


def test_the_multimodal_wrapper_is_refused_by_name_and_the_orderings_hold():
    from llamarec_amd import config as cfg
    from llamarec_amd.llm import GEMMA3_1B, GEMMA3_FAMILY, SUPPORTED_MODEL_TYPES, model_family

    with pytest.raises(NotImplementedError, match=r"multimodal.*gemma3_text.*gemma-3-1b"):
        model_family(dict(GEMMA3_1B, model_type="gemma3"))
    assert GEMMA3_FAMILY == ("gemma3_text",)
    t = SUPPORTED_MODEL_TYPES
    assert t[-1] == "gemma2" and t.index("qwen3") < t.index("gemma") < t.index("gemma3_text") < t.index("gemma2")
    assert cfg.LLM_CHOICES[:7] == ["llama2", "llama3", "phi3", "gemma", "mistral", "gemma2", "qwen2"]
    assert cfg.LLM_CHOICES[7] == "gemma3" and cfg.LLM_CHOICES[-1] == "qwen3"
    assert cfg.LLM_BASE_MODELS["gemma3"] == "google/gemma-3-1b-pt"
    a = cfg.parse(["--dataset_code", "beauty", "--llm", "gemma3"], model_code="llm")
    g = cfg.parse(["--dataset_code", "beauty", "--llm", "gemma"], model_code="llm")
    assert a.llm_base_model == a.llm_base_tokenizer == "google/gemma-3-1b-pt"
    assert (a.train_batch_size, a.lora_micro_batch_size, a.test_batch_size) == (g.train_batch_size, g.lora_micro_batch_size,
                                                                                g.test_batch_size) == (4, 2, 4)


def test_gemma3_preset_ranker_words_and_shapes():
    from llamarec_amd import _abi as A
    from llamarec_amd.llm import GEMMA3_1B, LlamaRanker

    c = GEMMA3_1B
    assert (c["vocab_size"], c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["num_attention_heads"],
            c["num_key_value_heads"], c["head_dim"], c["sliding_window"]) == (262144, 1152, 6912, 26, 4, 1, 256, 512)
    r = LlamaRanker(dict(c), device="cpu")
    assert r.family == "gemma3" and r.max_prompt_len is None       # nothing is refused for length
    r._check_lengths(np.array([0, 5000], np.int32))
    assert r.default_gemm_variant == 6 and r.rope_theta == 1e6 and r.rope_scaling is None
    arch = r.arch()
    assert (arch.norm_style, arch.mlp_act, arch.embed_scale) == (1, 1, 34.0)      # bf16(sqrt(1152)) = 34
    assert ctypes.sizeof(A.LrGemma3Ext) == 32 + 5 * ctypes.sizeof(ctypes.c_void_p)
    names = dict(gemma3_param_shapes(c))
    assert "lm_head.weight" not in names and len(names) == 2 + 26 * 13
    assert names["model.layers.3.self_attn.q_norm.weight"] == names["model.layers.3.self_attn.k_norm.weight"] == (256,)
    assert names["model.layers.0.self_attn.q_proj.weight"] == (1024, 1152)
    assert names["model.layers.25.pre_feedforward_layernorm.weight"] == (1152,)
    with pytest.raises(NotImplementedError, match="folded norms"):
        r.set_fold_norms(True)


def test_training_a_gemma3_base_is_refused_before_anything_is_loaded(tmp_path):
    import train_ranker

    with pytest.raises(SystemExit, match="LoRA fine-tuning needs a Llama-family base"):
        train_ranker.main(["--dataset_code", "beauty", "--llm", "gemma3", "--synthetic", "--llm_retrieved_path", str(tmp_path)])


# ---- the float64 references ---------------------------------------------------------------------------------------------
def test_window_reference_equals_a_dense_masked_softmax_at_tiny_sizes():
    nh, nkv, hd = 4, 2, 16
    lens = [1, 2, 7, 19]
    cu = np.concatenate([[0], np.cumsum(lens)])
    qkv = G3.window_data("peaked", cu, nh, nkv, hd)
    for W in (1, 2, 3, 7, 18, 19, 50):
        ref, bound = G3.attention_window_ref64(qkv, cu, nh, nkv, hd, W)
        assert np.abs(ref - G3.attention_dense_window(qkv, cu, nh, nkv, hd, W)).max() < 1e-12, W
        assert (bound > 0).all()
    one, _ = G3.attention_window_ref64(qkv, cu, nh, nkv, hd, 1)     # a window of one key: every row is its own value row
    v = qkv[:, (nh + nkv) * hd:].reshape(-1, nkv, hd)
    assert np.array_equal(one.reshape(-1, nh, hd), np.repeat(v, nh // nkv, axis=1))
    # the mask of the torch forward is the same relation
    m = G3.window_mask(6, 3).numpy()
    assert [(i, j) for i in range(6) for j in range(6) if m[i, j] == 0] == [(i, j) for i in range(6) for j in range(6)
                                                                            if i - 3 < j <= i]


def test_the_kernel_batches_meet_every_hazard_of_the_windowed_block_walk():
    from tests.test_gpu_attn_window import LAST_LENS, LENS, WINDOWS, spike_case

    assert set(WINDOWS) == {1, 16, 17, 63, 64, 65, 100, 128, 200}
    assert set(LENS) == {1, 15, 64, 65, 127, 128, 129, 200, 321, 450} and sum(LENS) <= 2000
    met = {}
    for W in WINDOWS:
        for k, v in G3.window_cases(LENS, W).items():
            met[k] = met.get(k, False) or v
    assert all(met.values()), met
    assert any(T == W + 1 for T in LENS for W in WINDOWS) and any(T <= W for T in LENS for W in WINDOWS)
    for W in WINDOWS:      # the last-row batch has prompts on both sides of every window and of the 64-key block
        assert min(LAST_LENS) <= min(W, 64) and max(LAST_LENS) > max(W, 64), W
    # the spike: in a block behind the tile's first visited one; the other key is the last one outside the window
    cu, row, key_in, key_out = spike_case(100)
    T = int(cu[2] - cu[1])
    first = max(0, (row // 128) * 128 - 100 + 1) // 64
    assert row < T and row - 100 < key_in <= row and key_in // 64 > first and key_out == row - 100 and key_out // 64 >= first


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_every_window_mutant_is_outside_the_bound_on_the_kernel_cases(regime):
    from tests.test_gpu_attn_window import LENS, MUTANT_W, cu_of

    nh, nkv, hd = 4, 1, 256
    cu = cu_of(LENS)
    qkv = G3.window_data(regime, cu, nh, nkv, hd)
    ref, bound = G3.attention_window_ref64(qkv, cu, nh, nkv, hd, MUTANT_W)
    assert G3.ratio(bf16_round(ref.astype(np.float32)), ref, bound) <= 0.5      # the reference's own rounding is well inside
    for m in G3.WINDOW_MUTANTS:
        mut, _ = G3.attention_window_ref64(qkv, cu, nh, nkv, hd, MUTANT_W, m)
        r = G3.ratio(mut, ref, bound)
        print(f"{regime} {m}: err / bound {r:.1f}")
        assert r > 1.0, (m, r)


@pytest.mark.parametrize("hd", [128, 256])
def test_the_sweeps_reference_and_its_llama_mutant(hd):
    from tests.test_gpu_gemma3_kernels import sweep_data

    x, w, pos, cos, sin, eps = sweep_data(hd)
    ref, bound = G3.qk_norm_rope_ref64(x, w, eps, pos, cos, sin)
    # against a plain restatement of one element pair
    r, h, i = 5, 1, 3
    a = x[r, h].astype(np.float64) / np.sqrt((x[r, h].astype(np.float64) ** 2).mean() + eps) * (1.0 + w.astype(np.float64))
    c, s = float(cos[pos[r], i]), float(sin[pos[r], i])
    assert abs(ref[r, h, 2 * i] - (a[2 * i] * c - a[2 * i + 1] * s)) < 1e-12
    assert abs(ref[r, h, 2 * i + 1] - (a[2 * i + 1] * c + a[2 * i] * s)) < 1e-12
    mut, _ = G3.qk_norm_rope_ref64(x, w, eps, pos, cos, sin, "llama_qk_norm")
    assert G3.ratio(mut, ref, bound) > 1.0


@pytest.mark.parametrize("name", GEMMA3_GOLDENS)
def test_every_model_mutant_is_ten_tolerances_from_the_golden(golden_dir, name):
    z, cfg, sd, seqs = load_gemma3_golden(golden_dir, name)
    assert cfg == gemma3_cfg_dict(name) and [len(s) for s in seqs] == GEMMA3_CONFIGS[name][2]
    W = cfg["sliding_window"]
    assert min(map(len, seqs)) < W < max(map(len, seqs)) and any(G3.layer_is_sliding(cfg)) and not all(G3.layer_is_sliding(cfg))
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    assert float(np.abs(z["logits_bf16"] - z["logits_fp32"]).max()) <= tol
    for m in G3.MODEL_MUTANTS:
        d = float(np.abs(z[f"mutant_{m}"] - z["logits_fp32"]).max())
        print(f"{name} {m}: {d / tol:.1f} tolerances")
        if m in WEAK_MUTANTS.get(name, ()):      # (tests/gen_goldens_gemma3.py says why, with the figures)
            continue
        assert d > 10 * tol, (m, d, tol)
    # prompts within the window see no window: those rows of the window mutants are the golden's own
    short = [b for b, s in enumerate(seqs) if len(s) <= W - 1]
    for m in G3.WINDOW_MUTANTS:
        assert np.array_equal(z[f"mutant_{m}"][short], z["logits_fp32"][short]), m


def test_the_archives_are_what_the_restatement_computes(golden_dir):
    """One archive, a few prompts: the stored logits are gemma3_ref's on the rebuilt weights (the generator is reproducible)."""
    import torch

    z, cfg, sd, seqs = load_gemma3_golden(golden_dir, "tiny_hd128")
    pick = [0, 2, 4]
    got = G3.last_logits(sd, cfg, [seqs[b] for b in pick], torch.float32)
    assert np.abs(got - z["logits_fp32"][pick]).max() < 1e-4
    assert cfg["layer_types"] == ["sliding_attention", "full_attention", "sliding_attention"]
    assert json.loads(str(np.load(os.path.join(golden_dir, "gemma3_tiny_hd256_linear.npz"))["config"]))["rope_scaling"] == {
        "rope_type": "linear", "factor": 8.0}
    c7 = gemma3_cfg_dict("tiny_hd256_mqa")
    assert c7["num_hidden_layers"] == 7 and G3.layer_is_sliding(c7) == [True] * 5 + [False, True]
    assert c7["hidden_size"] % 64 == 0 and c7["hidden_size"] % 256 != 0 and c7["sliding_window"] == 100
