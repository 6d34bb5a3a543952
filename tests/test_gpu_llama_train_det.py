"""GPU: deterministic mode of the ranker's LoRA step (lr_llama_lora_set_deterministic, LoraTrainEngine.set_deterministic,
train_ranker.py --deterministic). Run-to-run bit identity of loss, gradients and the optimizer trajectory on the three tiny
models (MFMA and generic attention backward, every chunk length of the token reductions), parity with the float64 restatement
(tests/lora_modules_ref.py) and with the default mode, independence of the side stream and of other handles in flight, the
ABI's workspace contract, and the entry point. Nothing here counts on the default mode being non-deterministic."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import lora_modules_ref as R
from tests import test_gpu_lora_modules as M

pytestmark = pytest.mark.gpu

QV = ("q_proj", "v_proj")
ALL7 = R.MODULES
SETS = {"qv": QV, "all7": ALL7}
NAMES = ("tiny_hd128", "tiny_hd16", "tiny_gqa")   # MFMA attention backward; generic; generic with grouped heads (head_dim 32)
RAGGED = [3, 70, 4, 129]                           # 206 tokens = 7 chunks of 32; a prompt shorter than a key block


def _load(golden_dir, name):
    from llamarec_amd.synth import synth_llama_state

    z = np.load(os.path.join(golden_dir, f"llama_lora_train_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    return z, cfg, synth_llama_state(cfg, int(z["weight_seed"]))


def _init(z, cfg, mods):
    """q|v: the golden's own adapters; all seven: the restatement's random ones (B != 0, so that A has a gradient)."""
    if mods == "qv":
        return {str(n): z["init/" + str(n)] for n in z["param_names"]}
    return R.random_adapters(cfg, 8, ALL7, seed=11)


def _engine(sd, cfg, lora, mods, det=True, **kw):
    eng = M._engine(sd, cfg, lora, SETS[mods], **kw)
    return eng.set_deterministic(True) if det else eng


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _run(sd, cfg, lora, mods, seqs, labels, calls=1, **kw):
    """A fresh deterministic engine, `calls` passes over the batch: (loss bits, gradient bits) of the last one."""
    eng = _engine(sd, cfg, lora, mods, **kw)
    for _ in range(calls):
        loss = eng.loss_and_grads(seqs, labels)
    assert eng.bad_targets == 0
    return _bits(loss), _bits(eng.grads), eng


def _same(a, b, tag):
    assert torch.equal(a[0], b[0]), (tag, "loss", a[0].item(), b[0].item())
    diff = int((a[1] != b[1]).sum())
    assert diff == 0, (tag, f"{diff} of {a[1].numel()} gradient words differ")


# ---- 1. run-to-run bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods", ["qv", "all7"])
@pytest.mark.parametrize("name", NAMES)
def test_two_runs_give_the_same_bits(golden_dir, name, mods):
    z, cfg, sd = _load(golden_dir, name)
    lora = _init(z, cfg, mods)
    seqs, labels = M._batch(cfg, RAGGED, 5)
    a = _run(sd, cfg, lora, mods, seqs, labels)
    b = _run(sd, cfg, lora, mods, seqs, labels)
    _same(a, b, "two engines")
    assert float(a[1].view(torch.float32).abs().max()) > 0
    again = a[2].loss_and_grads(seqs, labels)               # no dropout: the pass counter does not enter
    _same(a, (_bits(again), _bits(a[2].grads)), "same engine, second call")
    # dropout: the streams follow the pass counter, so the second run is a fresh engine as well
    c = _run(sd, cfg, lora, mods, seqs, labels, dropout=0.3, seed=9)
    d = _run(sd, cfg, lora, mods, seqs, labels, dropout=0.3, seed=9)
    _same(c, d, "dropout 0.3")
    assert not torch.equal(c[1], a[1])


@pytest.mark.parametrize("lens", [[200, 150, 140, 129], [250] * 17], ids=["619_tokens_chunk128", "4250_tokens_chunk256"])
def test_every_chunk_length_of_the_token_reductions(golden_dir, lens):
    """lt_tn_chunk: 32 below 512 tokens (the cases above), 128 from 512, 256 from 4096."""
    z, cfg, sd = _load(golden_dir, "tiny_hd128")
    lora = _init(z, cfg, "all7")
    seqs, labels = M._batch(cfg, lens, 7)
    _same(_run(sd, cfg, lora, "all7", seqs, labels), _run(sd, cfg, lora, "all7", seqs, labels), str(sum(lens)))


# ---- 2. parity: the restatement's bar, and the default mode of the same build ----------------------------------------------
@pytest.mark.parametrize("name", ["tiny_hd128", "tiny_gqa"])
def test_parity_with_float64_restatement_and_default_mode(golden_dir, name):
    z, cfg, sd = _load(golden_dir, name)
    lora = _init(z, cfg, "all7")
    seqs, labels = M._batch(cfg, RAGGED, 5)
    det = _engine(sd, cfg, lora, "all7")
    loss = float(det.loss_and_grads(seqs, labels))
    l64, g64, _ = R.loss_and_grads(sd, cfg, lora, seqs, labels, 8, 32)
    _, gbf, _ = R.loss_and_grads(sd, cfg, lora, seqs, labels, 8, 32, mode="bf16")
    assert det.bad_targets == 0
    assert abs(loss - l64) < 4e-3, (loss, l64)
    M._assert_grads(M._grads(det), g64, gbf, f"det/{name}")
    dflt = _engine(sd, cfg, lora, "all7", det=False)
    l0 = float(dflt.loss_and_grads(seqs, labels))
    worst = ((det.grads - dflt.grads).abs() / (1e-6 + 1e-3 * dflt.grads.abs())).max().item()
    print(f"det vs default {name}: loss {loss!r} / {l0!r}, worst |diff| / (atol + rtol |ref|) = {worst:.3f}")
    assert abs(loss - l0) < 1e-5
    assert torch.allclose(det.grads, dflt.grads, rtol=1e-3, atol=1e-6)


# ---- 3. scheduling does not matter -------------------------------------------------------------------------------------------
def test_side_stream_or_not_gives_the_same_bits(golden_dir, monkeypatch):
    """LR_LORA_OVERLAP is read at create: one handle with every kernel in order on the caller's stream, one with the side stream."""
    z, cfg, sd = _load(golden_dir, "tiny_gqa")
    lora = _init(z, cfg, "all7")
    seqs, labels = M._batch(cfg, RAGGED, 5)
    monkeypatch.setenv("LR_LORA_OVERLAP", "0")
    in_order = _run(sd, cfg, lora, "all7", seqs, labels)
    monkeypatch.delenv("LR_LORA_OVERLAP")
    overlapped = _run(sd, cfg, lora, "all7", seqs, labels)
    _same(in_order, overlapped, "LR_LORA_OVERLAP=0 vs side stream")


# ---- 4. handles are independent ----------------------------------------------------------------------------------------------
def test_handles_in_flight_on_two_streams_keep_their_solo_bits(golden_dir):
    z, cfg, sd = _load(golden_dir, "tiny_gqa")
    lora = _init(z, cfg, "all7")
    batch_a, batch_b = M._batch(cfg, RAGGED, 5), M._batch(cfg, [64, 5, 130], 6)
    a, b = _engine(sd, cfg, lora, "all7"), _engine(sd, cfg, lora, "all7", det=False)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def solo(eng, batch):
        eng.loss_and_grads(*batch)
        torch.cuda.synchronize()
        return _bits(eng.grads)

    def interleaved():
        torch.cuda.synchronize()
        for _ in range(2):                                   # A, B, A, B issued back to back; one synchronisation at the end
            with torch.cuda.stream(s1):
                a.loss_and_grads(*batch_a)
            with torch.cuda.stream(s2):
                b.loss_and_grads(*batch_b)
        torch.cuda.synchronize()
        return _bits(a.grads), _bits(b.grads)

    solo_a = solo(a, batch_a)
    got_a, _ = interleaved()                                 # A deterministic, B not
    assert torch.equal(got_a, solo_a)
    b.set_deterministic(True)
    solo_b = solo(b, batch_b)
    got_a, got_b = interleaved()                             # both deterministic
    assert torch.equal(got_a, solo_a) and torch.equal(got_b, solo_b)


# ---- 5. optimizer trajectory -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mods", [("tiny_hd16", "qv"), ("tiny_gqa", "all7")])
def test_optimizer_trajectory_repeats_bit_for_bit(golden_dir, name, mods):
    """Four optimizer steps on the golden's two batches, alternating; step 2 is two accumulated micro-batches. The limit 0.05
    makes the clipping really rescale (the norms are asserted to exceed it)."""
    z, cfg, sd = _load(golden_dir, name)
    lora = _init(z, cfg, mods)
    from tests.test_gpu_llama_train import _unpack

    batches = [_unpack(z, 0), _unpack(z, 1)]

    def run():
        eng = _engine(sd, cfg, lora, mods)
        norms = []
        for step in range(4):
            if step == 2:
                eng.loss_and_grads(*batches[0], grad_scale=0.5)
                eng.loss_and_grads(*batches[1], grad_scale=0.5, accumulate=True)
            else:
                eng.loss_and_grads(*batches[step % 2])
            norms.append(_bits(eng.apply(2e-4, max_grad_norm=0.05)))
        return _bits(eng.params), _bits(eng.m), _bits(eng.v), torch.stack(norms)

    one, two = run(), run()
    for tag, x, y in zip(("params", "m", "v", "norms"), one, two):
        assert torch.equal(x, y), tag
    assert float(one[3].view(torch.float32).min()) > 0.05


# ---- 6. ABI behaviour ----------------------------------------------------------------------------------------------------------
def test_abi_workspace_contract_and_switching_back(golden_dir):
    from llamarec_amd._lib import lib, stream_ptr
    from llamarec_amd.llm import pack_prompts
    from llamarec_amd.rank_train import loss_rows_and_targets

    L_ = lib()
    assert L_.lr_llama_lora_set_deterministic(None, 1) == -1            # LR_EINVAL
    z, cfg, sd = _load(golden_dir, "tiny_gqa")
    lora = _init(z, cfg, "all7")
    seqs, labels = M._batch(cfg, RAGGED, 5)
    eng = _engine(sd, cfg, lora, "all7", det=False)
    ids, cu = pack_prompts(seqs)
    rows, tgts = loss_rows_and_targets(seqs, labels)
    n, B, m = int(cu[-1]), len(seqs), len(rows)
    before = L_.lr_llama_lora_workspace_bytes(eng._h, n, B, m)
    eng.set_deterministic(True)
    after = L_.lr_llama_lora_workspace_bytes(eng._h, n, B, m)
    assert eng._ws is None and before > 0 and after >= before and after > before, (before, after)
    dev = eng.device
    dv = [torch.from_numpy(x).to(dev) for x in (ids, cu, rows, tgts)]
    small = torch.empty(before, dtype=torch.uint8, device=dev)
    rc = L_.lr_llama_lora_loss_grad(eng._h, dv[0].data_ptr(), dv[1].data_ptr(), cu.ctypes.data, B, dv[2].data_ptr(),
                                    dv[3].data_ptr(), m, 1.0, 0, eng._out.data_ptr(), small.data_ptr(), small.numel(),
                                    stream_ptr())
    assert rc == -4, rc                                                   # LR_EWORKSPACE
    torch.cuda.synchronize()                                              # nothing was launched, nothing faulted
    # a workspace sized for more tokens serves every smaller batch (the chunk count is not monotonic in the token count)
    assert L_.lr_llama_lora_workspace_bytes(eng._h, 512, B, m) >= L_.lr_llama_lora_workspace_bytes(eng._h, 511, B, m)
    eng.set_deterministic(False)
    assert L_.lr_llama_lora_workspace_bytes(eng._h, n, B, m) == before
    loss = float(eng.loss_and_grads(seqs, labels))
    l64, g64, _ = R.loss_and_grads(sd, cfg, lora, seqs, labels, 8, 32)
    _, gbf, _ = R.loss_and_grads(sd, cfg, lora, seqs, labels, 8, 32, mode="bf16")
    assert abs(loss - l64) < 4e-3
    M._assert_grads(M._grads(eng), g64, gbf, "switched back")


# ---- 7. entry point --------------------------------------------------------------------------------------------------------------
def test_train_ranker_deterministic_writes_the_same_adapter_twice(tmp_path):
    from safetensors import safe_open

    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    assert pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))["test_users"]
    results = []
    for run in ("one", "two"):
        root = str(tmp_path / run)
        metrics = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--deterministic", "--llm_retrieved_path",
                                     lru_root, "--export_root", root, "--lora_max_steps", "4", "--lora_val_iterations", "2",
                                     "--warmup_steps", "1", "--lora_micro_batch_size", "4", "--train_batch_size", "8",
                                     "--lora_max_val_samples", "16", "--llm_max_history", "5"])
        with safe_open(os.path.join(root, "adapter", "adapter_model.safetensors"), framework="pt") as f:
            results.append((metrics, {k: f.get_tensor(k) for k in f.keys()}))
    (m1, t1), (m2, t2) = results
    assert sorted(t1) == sorted(t2) and len(t1) == 8
    assert any(float(v.abs().max()) > 0 for k, v in t1.items() if "lora_B" in k)
    for k in t1:
        assert torch.equal(t1[k], t2[k]), k
    # the ranking metrics of both dictionaries; the evaluator also reports its own wall-clock time, which no mode can repeat
    clock = ("test_runtime", "test_samples_per_second")
    for d1, d2 in zip(m1, m2):
        assert sorted(d1) == sorted(d2) and any(k not in clock for k in d1)
        for k in d1:
            assert k in clock or d1[k] == d2[k], (k, d1[k], d2[k])
