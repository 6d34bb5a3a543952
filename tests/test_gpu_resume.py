"""GPU: resumable ranker fine-tuning. The two counters no buffer shows travel through the ABI (lr_llama_lora_get_progress /
lr_llama_lora_set_progress) and, with params / m / v, are everything a later step depends on; train_ranker.py resumed from
checkpoint-N writes the bits (--deterministic) of the run that was never interrupted, or stays inside the bar between the
default and the deterministic mode (tests/test_gpu_llama_train_det.py: rtol 1e-3, atol 1e-6) without the flag; a checkpoint is
a PEFT adapter directory."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import test_gpu_llama_train_det as D
from tests.test_gpu_llama_train import _unpack

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-3, 1e-6       # default vs deterministic trajectories, tests/test_gpu_llama_train_det.py
CLOCK = ("test_runtime", "test_samples_per_second")


def _three_steps(eng, batches):
    """Three optimizer steps, the second accumulated over two passes: 3 steps, 4 passes."""
    eng.loss_and_grads(*batches[0])
    eng.apply(2e-4, max_grad_norm=0.05)
    eng.loss_and_grads(*batches[0], grad_scale=0.5)
    eng.loss_and_grads(*batches[1], grad_scale=0.5, accumulate=True)
    eng.apply(2e-4, max_grad_norm=0.05)
    eng.loss_and_grads(*batches[1])
    eng.apply(2e-4, max_grad_norm=0.05)


def _step4(eng, batches):
    loss = D._bits(eng.loss_and_grads(*batches[0]))
    eng.apply(2e-4, max_grad_norm=0.05)
    return loss, D._bits(eng.params), D._bits(eng.m), D._bits(eng.v)


# ---- 1. counters through the ABI --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods", ["qv", "all7"])
@pytest.mark.parametrize("name", ["tiny_hd16", "tiny_gqa"])
def test_state_dict_with_the_counters_continues_with_the_same_bits(golden_dir, name, mods):
    z, cfg, sd = D._load(golden_dir, name)
    lora = D._init(z, cfg, mods)
    batches = [_unpack(z, 0), _unpack(z, 1)]
    kw = dict(dropout=0.3, seed=9)
    a = D._engine(sd, cfg, lora, mods, **kw)
    assert a.progress() == (0, 0)
    _three_steps(a, batches)
    assert a.progress() == (3, 4)
    state = a.state_dict()
    assert (state["optimizer_steps"], state["passes"]) == (3, 4)
    assert all(state[k].device.type == "cpu" and state[k].dtype == torch.float32 and state[k].numel() == state["n_params"]
               for k in ("params", "exp_avg", "exp_avg_sq"))
    assert state["target_modules"] == list(D.SETS[mods]) and (state["r"], state["dropout"], state["seed"]) == (8, 0.3, 9)
    assert state["hidden_size"] == cfg["hidden_size"] and state["num_key_value_heads"] == cfg["num_key_value_heads"]
    assert float(state["exp_avg_sq"].max()) > 0
    want = _step4(a, batches)
    assert a.progress() == (4, 5)

    b = D._engine(sd, cfg, lora, mods, **kw).load_state_dict(state)
    assert b.deterministic and b.progress() == (3, 4)
    got = _step4(b, batches)
    for tag, x, y in zip(("loss", "params", "m", "v"), want, got):
        assert torch.equal(x, y), (tag, int((x != y).sum()))

    c = D._engine(sd, cfg, lora, mods, **kw)                      # the three buffers, not the counters
    c.params.copy_(state["params"]), c.m.copy_(state["exp_avg"]), c.v.copy_(state["exp_avg_sq"])
    other = _step4(c, batches)
    assert c.progress() == (1, 1)
    assert not torch.equal(other[0], want[0])                     # pass 1's dropout masks, not pass 5's
    assert not torch.equal(other[1], want[1])                     # and step 1's bias correction


def test_load_state_dict_refuses_another_layout_by_the_name_of_the_field(golden_dir):
    z, cfg, sd = D._load(golden_dir, "tiny_hd16")
    state = D._engine(sd, cfg, D._init(z, cfg, "qv"), "qv", dropout=0.3, seed=9).state_dict()
    for field, mods, kw in (("target_modules", "all7", dict(dropout=0.3, seed=9)), ("seed", "qv", dict(dropout=0.3, seed=10)),
                            ("dropout", "qv", dict(dropout=0.1, seed=9))):
        eng = D._engine(sd, cfg, D._init(z, cfg, mods), mods, **kw)
        before = D._bits(eng.params)
        with pytest.raises(ValueError, match=field):
            eng.load_state_dict(state)
        assert torch.equal(before, D._bits(eng.params)) and eng.progress() == (0, 0)
    z2, cfg2, sd2 = D._load(golden_dir, "tiny_gqa")
    with pytest.raises(ValueError, match="n_params|num_|head_dim|hidden_size|intermediate_size"):
        D._engine(sd2, cfg2, D._init(z2, cfg2, "qv"), "qv", dropout=0.3, seed=9).load_state_dict(state)


# ---- 2. bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_progress_arguments_are_refused_and_the_handle_trains_on(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd._lib import lib, stream_ptr

    L_ = lib()
    z, cfg, sd = D._load(golden_dir, "tiny_hd16")
    batches = [_unpack(z, 0), _unpack(z, 1)]
    eng = D._engine(sd, cfg, D._init(z, cfg, "qv"), "qv")
    eng.loss_and_grads(*batches[0])
    eng.apply(2e-4)
    ok = A.LrLoraProgress(optimizer_steps=1, passes=1)
    bad = [("null argument", lambda: L_.lr_llama_lora_set_progress(eng._h, None, stream_ptr())),
           ("null argument", lambda: L_.lr_llama_lora_get_progress(eng._h, None, stream_ptr())),
           ("null argument", lambda: L_.lr_llama_lora_set_progress(None, C.byref(ok), stream_ptr())),
           ("negative", lambda: L_.lr_llama_lora_set_progress(eng._h, C.byref(A.LrLoraProgress(optimizer_steps=-1, passes=1)),
                                                              stream_ptr())),
           ("negative", lambda: L_.lr_llama_lora_set_progress(eng._h, C.byref(A.LrLoraProgress(optimizer_steps=1, passes=-2)),
                                                              stream_ptr())),
           ("step counter", lambda: L_.lr_llama_lora_set_progress(
               eng._h, C.byref(A.LrLoraProgress(optimizer_steps=2 ** 31, passes=1)), stream_ptr())),
           ("pass counter", lambda: L_.lr_llama_lora_set_progress(
               eng._h, C.byref(A.LrLoraProgress(optimizer_steps=1, passes=2 ** 32)), stream_ptr())),
           ("reserved", lambda: L_.lr_llama_lora_set_progress(
               eng._h, C.byref(A.LrLoraProgress(optimizer_steps=1, passes=1, reserved=(C.c_int64 * 2)(0, 7))), stream_ptr()))]
    for word, call in bad:
        assert call() == -1, word                                                  # LR_EINVAL
        assert word.encode() in L_.lr_last_error(), (word, L_.lr_last_error())
        assert eng.progress() == (1, 1), word                                      # unchanged
    # the widest values the counter types hold are accepted, and reported back
    eng.set_progress(2 ** 31 - 1, 2 ** 32 - 1)
    assert eng.progress() == (2 ** 31 - 1, 2 ** 32 - 1)
    eng.set_progress(1, 1)
    loss = float(eng.loss_and_grads(*batches[1]))
    norm = float(eng.apply(2e-4))
    assert np.isfinite(loss) and norm > 0 and eng.bad_targets == 0 and eng.progress() == (2, 2)


# ---- 3. / 4. the entry point ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lru_root(tmp_path_factory):
    import train_retriever

    root = str(tmp_path_factory.mktemp("resume") / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    assert pickle.load(open(os.path.join(root, "retrieved.pkl"), "rb"))["test_users"]
    return root


def _flags(lru_root, root, det, modules):
    return (["--dataset_code", "synthetic", "--synthetic", "--llm_retrieved_path", lru_root, "--export_root", root,
             "--lora_max_steps", "6", "--lora_val_iterations", "2", "--lora_save_steps", "2", "--warmup_steps", "1",
             "--lora_micro_batch_size", "4", "--train_batch_size", "8", "--lora_max_val_samples", "16", "--llm_max_history", "5"]
            + (["--deterministic"] if det else []) + (["--lora_target_modules", "all-linear"] if modules == "all-linear" else []))


_RUNS = {}


def _run_a(lru_root, tmp_path_factory, det, modules):
    """The uninterrupted run, once per (mode, modules); later tests only read it."""
    import train_ranker

    if (det, modules) not in _RUNS:
        root = str(tmp_path_factory.mktemp(f"a_{'det' if det else 'default'}_{modules}"))
        _RUNS[det, modules] = (root, train_ranker.main(_flags(lru_root, root, det, modules)))
    return _RUNS[det, modules]


def _tensors(path):
    from safetensors import safe_open

    with safe_open(path, framework="pt") as f:
        return {k: f.get_tensor(k) for k in f.keys()}


def _pair(lru_root, tmp_path_factory, tmp_path, det, modules):
    import train_ranker

    root_a, metrics_a = _run_a(lru_root, tmp_path_factory, det, modules)
    assert sorted(d for d in os.listdir(root_a) if d.startswith("checkpoint")) == ["checkpoint-2", "checkpoint-4", "checkpoint-6"]
    root_b = str(tmp_path / "b")
    metrics_b = train_ranker.main(_flags(lru_root, root_b, det, modules)
                                  + ["--resume_from_checkpoint", os.path.join(root_a, "checkpoint-2")])
    assert sorted(d for d in os.listdir(root_b) if d.startswith("checkpoint")) == ["checkpoint-4", "checkpoint-6"]
    files = [os.path.join("adapter", "adapter_model.safetensors"), os.path.join("checkpoint-6", "adapter_model.safetensors"),
             os.path.join("checkpoint-6", "optimizer.safetensors")]
    pairs = [(f, _tensors(os.path.join(root_a, f)), _tensors(os.path.join(root_b, f))) for f in files]
    n = 2 * 2 * (7 if modules == "all-linear" else 2)
    assert len(pairs[0][1]) == len(pairs[1][1]) == n and sorted(pairs[2][1]) == ["exp_avg", "exp_avg_sq"]
    assert any(float(v.abs().max()) > 0 for k, v in pairs[1][1].items() if "lora_B" in k)
    assert float(pairs[2][1]["exp_avg_sq"].max()) > 0
    for f, ta, tb in pairs:
        assert sorted(ta) == sorted(tb), f
    return root_a, root_b, metrics_a, metrics_b, pairs


@pytest.mark.parametrize("modules", ["default", "all-linear"])
def test_train_ranker_resumed_deterministic_run_writes_the_uninterrupted_bits(lru_root, tmp_path_factory, tmp_path, modules):
    root_a, root_b, metrics_a, metrics_b, pairs = _pair(lru_root, tmp_path_factory, tmp_path, True, modules)
    for f, ta, tb in pairs:
        for k in ta:
            assert torch.equal(ta[k], tb[k]), (f, k, int((ta[k] != tb[k]).sum()))
    ha, hb = (json.load(open(os.path.join(r, "lora_eval_history.json"))) for r in (root_a, root_b))
    assert ha == hb and [h["step"] for h in ha] == [2, 4, 6]
    for d1, d2 in zip(metrics_a, metrics_b):
        assert sorted(d1) == sorted(d2) and any(k not in CLOCK for k in d1)
        for k in d1:
            assert k in CLOCK or d1[k] == d2[k], (k, d1[k], d2[k])
    sa, sb = (json.load(open(os.path.join(r, "checkpoint-6", "trainer_state.json"))) for r in (root_a, root_b))
    assert sa == sb and sa["optimizer_steps"] == 6 and sa["passes"] >= 6
    assert json.load(open(os.path.join(root_a, "checkpoint-6", "rng_state_0.json"))) == \
        json.load(open(os.path.join(root_b, "checkpoint-6", "rng_state_0.json")))


@pytest.mark.parametrize("modules", ["default", "all-linear"])
def test_train_ranker_resumed_default_run_stays_inside_the_modes_bar(lru_root, tmp_path_factory, tmp_path, modules):
    """The bar is the one between the default and the deterministic mode of ONE pass; this test holds six-step trajectories of
    the default mode to it, as the contract asks. Measured on an MI355X, worst |diff| / (atol + rtol |ref|) over the tensors of
    checkpoint-6 (adapter / optimizer), four runs each against one uninterrupted run:
      q_proj | v_proj   uninterrupted again 0.001 / 0.001     resumed from checkpoint-2  0.000 / 0.000   -- inside the bar
      all-linear        uninterrupted again 0.000 / 0.001 in two runs, 2.552 / 11.316 and 3.247 / 10.435 in the other two
                        resumed             0.000 / 0.000 in two runs, 2.552 / 11.316 in the other two   -- MISSES the bar
    With all seven modules the default mode itself takes one of a few discrete trajectories from run to run (its fp32 atomics
    add in another order, and the bf16 working copies of the adapters can turn one fp32 ulp into one bf16 ulp): two
    UNINTERRUPTED runs miss this bar against each other as often, and by the same figures, as a resumed one does. The resumed
    run adds nothing to that spread (the deterministic test above is bit-exact), but the all-linear case of this test fails
    whenever the two runs land on different trajectories -- about every second run."""
    root_a, root_b, _, _, pairs = _pair(lru_root, tmp_path_factory, tmp_path, False, modules)
    for f, ta, tb in pairs:
        worst = max(((ta[k] - tb[k]).abs() / (ATOL + RTOL * ta[k].abs())).max().item() for k in ta)
        print(f"resumed vs uninterrupted, default mode, {modules}, {f}: worst |diff| / (atol + rtol |ref|) = {worst:.3f}")
    for f, ta, tb in pairs:
        for k in ta:
            assert torch.allclose(tb[k], ta[k], rtol=RTOL, atol=ATOL), (f, k)


# ---- 5. a checkpoint is an adapter -----------------------------------------------------------------------------------------------------
def test_a_checkpoint_loads_and_scores_as_a_peft_adapter(lru_root, tmp_path_factory, tmp_path):
    import train_ranker
    from llamarec_amd.llm import load_peft_adapter

    root_a, _ = _run_a(lru_root, tmp_path_factory, True, "default")
    ck = os.path.join(root_a, "checkpoint-4")
    lora = load_peft_adapter(ck)
    saved = _tensors(os.path.join(ck, "adapter_model.safetensors"))
    assert (lora["r"], lora["alpha"], tuple(lora["target_modules"])) == (8, 32, ("q_proj", "v_proj")) and len(saved) == 8
    for k, v in saved.items():
        assert np.array_equal(lora["weights"][k.replace("base_model.model.", "", 1)], v.numpy()), k
    assert not all(torch.equal(v, _tensors(os.path.join(root_a, "checkpoint-6", "adapter_model.safetensors"))[k])
                   for k, v in saved.items())                                   # step 4's tensors, not the last ones
    subset, overall = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm_retrieved_path", lru_root,
                                         "--export_root", str(tmp_path / "eval"), "--eval_only", "--llm_adapter_path", ck,
                                         "--llm_max_history", "5"])
    ranking = {k: v for k, v in subset.items() if k not in CLOCK}
    assert ranking and all(np.isfinite(v) for v in ranking.values()) and sorted(ranking) == sorted(
        k for k in _run_a(lru_root, tmp_path_factory, True, "default")[1][0] if k not in CLOCK)
