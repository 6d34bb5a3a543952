"""Host side of resumable ranker fine-tuning (no GPU): LoraRankerTrainer's checkpoint-<step> directories -- write, rotate,
find the last, refuse a run that differs, continue exactly -- over the stand-in engine of tests/resume_fakes.py; the flags;
the two ABI symbols' declarations and their argument checks, which run before anything touches a device."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from tests import resume_fakes as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _listing(root):
    return sorted(os.listdir(root))


def _step6(root):
    """The parameters after step 6 (train() ends by loading the best ones, which may be an earlier step's)."""
    from safetensors.torch import load_file

    return load_file(os.path.join(root, "checkpoint-6", "adapter_model.safetensors"))["flat"]


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """The uninterrupted run every resumed one is compared with: 6 steps, checkpoints 2 / 4 / 6. Left unchanged."""
    root = str(tmp_path_factory.mktemp("run_a"))
    tr, eng = F.make_trainer(F.lora_args(), root)
    assert tr.train() == 6
    return root, tr, eng


# ---- 1. straight against resumed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [2, 4])
def test_resumed_run_reaches_the_uninterrupted_run(run_a, tmp_path, at):
    root_a, tr_a, eng_a = run_a
    assert _listing(root_a) == ["adapter", "best_adapter", "checkpoint-2", "checkpoint-4", "checkpoint-6",
                                "lora_eval_history.json"]
    ck = os.path.join(root_a, f"checkpoint-{at}")
    assert _listing(ck) == ["adapter_config.json", "adapter_model.safetensors", "best_adapter_model.safetensors",
                            "optimizer.safetensors", "rng_state_0.json", "trainer_state.json"]
    st = json.load(open(os.path.join(ck, "trainer_state.json")))
    assert (st["global_step"], st["optimizer_steps"], st["passes"]) == (at, at, 2 * at)
    assert (st["epoch"], st["step_in_epoch"]) == {2: (0, 2), 4: (0, 4)}[at]      # step 4 is the last of epoch 0
    assert [h["step"] for h in st["log_history"]] == list(range(2, at + 1, 2))
    assert st["fingerprint"]["world_size"] == 1 and st["engine"]["r"] == 8

    root_b = str(tmp_path / "b")
    tr_b, eng_b = F.make_trainer(F.lora_args(resume_from_checkpoint=ck), root_b)
    assert tr_b.train() == 6
    for name in ("params", "m", "v"):
        assert torch.equal(getattr(eng_a, name), getattr(eng_b, name)), name
    assert (eng_a.steps, eng_a.passes) == (eng_b.steps, eng_b.passes) == (6, 12)
    assert tr_a.history == tr_b.history and len(tr_a.history) == 3
    assert (tr_a.best_metric, tr_a.bad_evals) == (tr_b.best_metric, tr_b.bad_evals)
    assert json.load(open(os.path.join(root_a, "lora_eval_history.json"))) == \
        json.load(open(os.path.join(root_b, "lora_eval_history.json")))
    assert len(eng_b.seen) == 2 * (6 - at) and eng_a.seen[2 * at:] == eng_b.seen        # the samples of every later pass
    assert {i for p in eng_a.seen[:8] for i, _ in p} & {i for p in eng_a.seen[8:] for i, _ in p}   # epoch 1 revisits samples
    # B wrote the later checkpoints itself, with A's contents
    from safetensors.torch import load_file

    assert [d for d in _listing(root_b) if d.startswith("checkpoint-")] == [f"checkpoint-{s}" for s in range(at + 2, 7, 2)]
    for f in ("adapter_model.safetensors", "optimizer.safetensors", "best_adapter_model.safetensors"):
        a, b = (load_file(os.path.join(r, "checkpoint-6", f)) for r in (root_a, root_b))
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a), f
    sa, sb = (json.load(open(os.path.join(r, "checkpoint-6", "trainer_state.json"))) for r in (root_a, root_b))
    assert sa == sb
    assert json.load(open(os.path.join(root_a, "checkpoint-6", "rng_state_0.json"))) == \
        json.load(open(os.path.join(root_b, "checkpoint-6", "rng_state_0.json")))


def test_without_the_sampler_state_the_samples_differ(run_a, tmp_path):
    """The comparison above can see the generator: a source whose generator the trainer does not find restarts it."""
    root_a, _, eng_a = run_a
    ck = os.path.join(root_a, "checkpoint-2")
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint=ck), str(tmp_path / "b"), samples=F.FakeSamplesHiddenRng(11))
    assert tr.train() == 6
    assert [[i for i, _ in p] for p in eng.seen] == [[i for i, _ in p] for p in eng_a.seen[4:]]   # the same sample indices ...
    assert eng.seen != eng_a.seen[4:]                                                              # ... drawn differently
    assert not torch.equal(_step6(str(tmp_path / "b")), _step6(root_a))
    assert not os.path.exists(os.path.join(str(tmp_path / "b"), "checkpoint-4", "rng_state_0.json"))   # no rng: no file
    # and a source WITH a generator refuses a checkpoint that lacks its file
    with pytest.raises(SystemExit, match="rng_state_0.json"):
        F.make_trainer(F.lora_args(resume_from_checkpoint=os.path.join(str(tmp_path / "b"), "checkpoint-4")),
                       str(tmp_path / "c"))[0].train()


def test_counters_and_moments_are_part_of_the_state(run_a, tmp_path):
    """The stand-in's step depends on m, v and both counters, as the HIP step does: dropping any changes the end."""
    root_a, _, eng_a = run_a
    ck = os.path.join(root_a, "checkpoint-2")
    for drop in ("exp_avg", "exp_avg_sq", "optimizer_steps", "passes"):
        tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint=ck), str(tmp_path / drop))
        load = eng.load_state_dict

        def without(sd, drop=drop, load=load):
            sd = dict(sd)
            sd[drop] = torch.zeros_like(sd[drop]) if isinstance(sd[drop], torch.Tensor) else 0
            return load(sd)

        eng.load_state_dict = without
        assert tr.train() == 6
        assert not torch.equal(_step6(str(tmp_path / drop)), _step6(root_a)), drop


def test_a_checkpoint_past_the_patience_finishes_at_once(run_a, tmp_path):
    root_a, tr_a, _ = run_a
    ck = os.path.join(root_a, "checkpoint-4")
    bad = json.load(open(os.path.join(ck, "trainer_state.json")))["bad_evals"]
    root = str(tmp_path / "b")
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint=ck, lora_early_stopping_patience=max(bad, 0)), root)
    assert tr.train() == 4 and eng.seen == []
    assert torch.equal(eng.params, tr.best_state) and os.path.isdir(os.path.join(root, "adapter"))


# ---- 2. rotation ----------------------------------------------------------------------------------------------------------------
def test_rotation_keeps_the_newest(tmp_path):
    root = str(tmp_path)
    F.make_trainer(F.lora_args(lora_save_total_limit=2), root)[0].train()
    assert [d for d in _listing(root) if d.startswith("checkpoint")] == ["checkpoint-4", "checkpoint-6"]
    # by step NUMBER: checkpoint-10 is newer than checkpoint-8
    root = str(tmp_path / "long")
    F.make_trainer(F.lora_args(lora_save_total_limit=2, lora_max_steps=11, lora_save_steps=2, lora_val_iterations=100), root)[0].train()
    assert [d for d in _listing(root) if d.startswith("checkpoint")] == ["checkpoint-10", "checkpoint-11"]   # 11: the last step


# ---- 3. "last" --------------------------------------------------------------------------------------------------------------------
def test_last_picks_the_highest_complete_checkpoint(run_a, tmp_path):
    import shutil

    from llamarec_amd.rank_train import list_checkpoints

    root_a, _, eng_a = run_a
    root = str(tmp_path / "r")
    shutil.copytree(root_a, root)
    shutil.rmtree(os.path.join(root, "checkpoint-6"))
    assert [s for s, _ in list_checkpoints(root)] == [2, 4]
    os.makedirs(os.path.join(root, "checkpoint-10.tmp"))                       # a write that did not finish
    json.dump({}, open(os.path.join(root, "checkpoint-10.tmp", "trainer_state.json"), "w"))
    os.makedirs(os.path.join(root, "checkpoint-8"))                            # no trainer_state.json
    os.makedirs(os.path.join(root, "checkpoint-best"))                         # no step number
    assert [s for s, _ in list_checkpoints(root)] == [2, 4]
    logs = []
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint="last"), root, log=lambda *a: logs.append(" ".join(map(str, a))))
    assert tr.resolve_checkpoint() == os.path.join(root, "checkpoint-4")
    assert tr.train() == 6 and len(eng.seen) == 4 and torch.equal(_step6(root), _step6(root_a))
    assert any("resumed from" in l and "checkpoint-4" in l for l in logs)


def test_last_with_an_empty_root_starts_fresh(run_a, tmp_path):
    _, _, eng_a = run_a
    logs = []
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint="last"), str(tmp_path), log=lambda *a: logs.append(" ".join(map(str, a))))
    assert tr.train() == 6 and len(eng.seen) == 12 and torch.equal(_step6(str(tmp_path)), _step6(run_a[0]))
    assert sum("starting fresh" in l for l in logs) == 1


# ---- 4. explicit path -----------------------------------------------------------------------------------------------------------
def test_an_explicit_path_that_is_missing_or_incomplete_exits(tmp_path):
    with pytest.raises(SystemExit, match="checkpoint-9"):
        F.make_trainer(F.lora_args(resume_from_checkpoint=str(tmp_path / "checkpoint-9")), str(tmp_path / "b"))[0].train()
    os.makedirs(str(tmp_path / "checkpoint-3"))
    with pytest.raises(SystemExit, match="trainer_state.json"):
        F.make_trainer(F.lora_args(resume_from_checkpoint=str(tmp_path / "checkpoint-3")), str(tmp_path / "b"))[0].train()


# ---- 5. a run that differs is refused by the name of the field -----------------------------------------------------------------------
@pytest.mark.parametrize("field,kw,world", [("world_size", {}, 2), ("lora_micro_batch_size", dict(micro=2), 1),
                                            ("seed", dict(seed=4), 1), ("lora_token_budget", dict(lora_token_budget=16384), 1),
                                            ("train_batch_size", dict(batch=16), 1), ("lora_lr", dict(lora_lr=0.2), 1)])
def test_fingerprint_mismatch_exits_naming_the_field(run_a, tmp_path, field, kw, world):
    ck = os.path.join(run_a[0], "checkpoint-2")
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint=ck, **kw), str(tmp_path), world=world)
    with pytest.raises(SystemExit) as e:
        tr.train()
    msg = str(e.value)
    mine, theirs = tr.fingerprint()[field], json.load(open(os.path.join(ck, "trainer_state.json")))["fingerprint"][field]
    assert field in msg and repr(mine) in msg and repr(theirs) in msg and mine != theirs
    assert eng.seen == [] and eng.steps == 0


@pytest.mark.parametrize("field,kw", [("r", dict(r=4)), ("target_modules", dict(target_modules=("q_proj", "k_proj", "v_proj")))])
def test_layout_mismatch_raises_naming_the_field(run_a, tmp_path, field, kw):
    ck = os.path.join(run_a[0], "checkpoint-2")
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint=ck), str(tmp_path), engine=F.FakeEngine(**kw))
    with pytest.raises(ValueError, match=field):
        tr.train()


def test_check_layout_names_every_field_of_the_real_engine():
    from llamarec_amd.rank_train import LoraTrainEngine, check_layout

    mine = dict(r=8, alpha=32.0, dropout=0.05, seed=42, target_modules=["q_proj", "v_proj"], n_params=100,
                **{k: 2 for k in LoraTrainEngine.LAYOUT_BASE_FIELDS})
    check_layout(mine, dict(mine, extra=1))
    for k in mine:
        other = dict(mine, **{k: ["q_proj"] if k == "target_modules" else mine[k] + 1})
        with pytest.raises(ValueError, match=k):
            check_layout(mine, other)
        with pytest.raises(ValueError, match=k):
            check_layout(mine, {j: v for j, v in mine.items() if j != k})


def test_another_lora_max_steps_is_accepted(run_a, tmp_path):
    ck = os.path.join(run_a[0], "checkpoint-2")
    tr, eng = F.make_trainer(F.lora_args(resume_from_checkpoint=ck, lora_max_steps=5, lora_save_steps=0,
                                         lora_val_iterations=100, lora_early_stopping_patience=3), str(tmp_path))
    assert tr.train() == 5 and len(eng.seen) == 6


# ---- 6. flags ---------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_a_run_without_them(tmp_path):
    from llamarec_amd import config

    base = ["--dataset_code", "synthetic", "--llm_retrieved_path", "x"]
    a = config.parse(base, model_code="llm")
    assert (a.lora_save_steps, a.lora_save_total_limit, a.resume_from_checkpoint) == (0, 3, None)
    a = config.parse(base + ["--lora_save_steps", "50", "--lora_save_total_limit", "5", "--resume_from_checkpoint", "last"],
                     model_code="llm")
    assert (a.lora_save_steps, a.lora_save_total_limit, a.resume_from_checkpoint) == (50, 5, "last")
    # a namespace that has never heard of the flags (tests/test_dist_gloo.py builds one): today's outputs, nothing else
    args = F.lora_args()
    for k in ("lora_save_steps", "lora_save_total_limit", "resume_from_checkpoint"):
        delattr(args, k)
    root = str(tmp_path)
    tr, eng = F.make_trainer(args, root)
    state_dicts = []
    eng.state_dict = lambda: state_dicts.append(1)
    assert tr.train() == 6
    assert _listing(root) == ["adapter", "best_adapter", "lora_eval_history.json"] and state_dicts == []
    # with the flag, steps that write no checkpoint make no engine call either: 6 steps, a save every 4 and at the end
    tr, eng = F.make_trainer(F.lora_args(lora_save_steps=4), str(tmp_path / "every4"))
    calls, sd = [], eng.state_dict
    eng.state_dict = lambda: (calls.append(eng.steps), sd())[1]
    tr.train()
    assert calls == [4, 6]


def test_entry_point_refuses_resume_with_eval_only_or_an_adapter(tmp_path):
    import train_ranker

    base = ["--dataset_code", "synthetic", "--synthetic", "--llm_retrieved_path", str(tmp_path), "--resume_from_checkpoint", "last"]
    for extra in (["--eval_only"], ["--llm_adapter_path", str(tmp_path)]):
        with pytest.raises(SystemExit, match="resume_from_checkpoint"):
            train_ranker.main(base + extra)


# ---- the two ABI symbols ----------------------------------------------------------------------------------------------------------
def test_progress_symbols_are_declared_bound_and_check_their_arguments():
    from llamarec_amd import _abi as A
    from llamarec_amd import _lib

    for name in ("lr_llama_lora_get_progress", "lr_llama_lora_set_progress"):
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and args == [C.c_void_p, C.POINTER(A.LrLoraProgress), C.c_void_p]
    assert C.sizeof(A.LrLoraProgress) == 32
    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    assert re.search(r"typedef struct LrLoraProgress \{\s*int64_t optimizer_steps;\s*int64_t passes;\s*int64_t reserved\[2\];\s*\} "
                     r"LrLoraProgress;", header)
    assert re.search(r"int lr_llama_lora_get_progress\(lr_llama_lora_t\* h, LrLoraProgress\* out, void\* hip_stream\);", header)
    assert re.search(r"int lr_llama_lora_set_progress\(lr_llama_lora_t\* h, const LrLoraProgress\* in, void\* hip_stream\);", header)
    L_, p = _lib.lib(), A.LrLoraProgress()
    for call in (L_.lr_llama_lora_get_progress, L_.lr_llama_lora_set_progress):     # a null handle: refused before any HIP call
        assert call(None, C.byref(p), None) == -1 and b"null argument" in L_.lr_last_error()
