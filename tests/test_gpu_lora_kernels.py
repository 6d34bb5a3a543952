"""GPU: the small kernels of the ranker's LoRA step (csrc/llama_train.hip), one at a time through their stand-alone entry
points, against the float64 references of tests/lora_kernels_ref.py, element by element within the bounds derived there. The
cases are that module's lists: the smallest shapes that reach every arm of every launcher. Outputs start NaN-poisoned (or, where
a kernel accumulates, pre-filled), guard rows and columns around every strided output must keep their bits, exact operand kinds
must come back bit for bit, and every bound test prints max(err / bound)."""
import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, f32_to_bf16_bits
from tests import lora_kernels_ref as K

pytestmark = pytest.mark.gpu

POISON = 0x7FC0          # a bf16 NaN
GUARD32 = 12345.5        # fp32 guard value


def _L():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def _bits(x):
    return torch.from_numpy(f32_to_bf16_bits(np.ascontiguousarray(x, dtype=np.float32)).view(np.int16))


def _buf(x, ld=None, guard_rows=1, col0=0):
    """bf16 device buffer [rows + guard_rows][ld] of NaN bits with x at columns col0.. of the first rows."""
    rows, cols = x.shape
    ld = cols if ld is None else ld
    b = torch.full((rows + guard_rows, ld), POISON, dtype=torch.int16)
    b[:rows, col0:col0 + cols] = _bits(x)
    return b.cuda()


def _f(t):
    return bf16_bits_to_f32(t.cpu().numpy().view(np.uint16))


def _poison_kept(t, written):
    """every element of the int16 buffer t outside the boolean mask `written` still holds the NaN bits"""
    b = t.cpu().numpy().view(np.uint16)
    return bool((b[~written] == POISON).all())


def _f32buf(x, guard=8):
    b = torch.full((x.size + guard,), GUARD32, dtype=torch.float32)
    b[:x.size] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(-1))
    return b.cuda()


def _ok(rc):
    from llamarec_amd._lib import lib

    assert rc == 0, (rc, lib().lr_last_error())


# ---- rank-r product ----------------------------------------------------------------------------------------------------------
def test_skinny_within_bound_exact_bit_for_bit_guards_kept():
    l, st = _L()
    worst, bad = 0.0, []
    for c in K.skinny_cases():
        n, Kk, nt, ocol = c["n"], c["K"], c["nt"], c["ocol"]
        x, w = K.skinny_data(c)
        xb, wb = _buf(x, Kk + 8), _buf(w, guard_rows=0)
        out = torch.full((n + 1, 48), POISON, dtype=torch.int16, device="cuda")
        _ok(l.lr_lora_skinny_bf16(xb.data_ptr(), Kk + 8, n, Kk, wb.data_ptr(), nt, out.data_ptr(), 48, ocol, c["scale"], K.STREAM,
                                  c["p"], st))
        torch.cuda.synchronize()
        written = np.zeros((n + 1, 48), bool)
        written[:n, ocol:ocol + 16 * nt] = True
        assert _poison_kept(out, written), ("guard rows / columns written", c)
        got = _f(out)[:n, ocol:ocol + 16 * nt]
        ref, bound = K.skinny_ref64(x, w, c["scale"], K.STREAM, c["p"])
        r = K.ratio(got, ref, bound)
        worst = max(worst, r)
        if r > 1.0:
            bad.append((c, r))
        if c["kind"] == "exact":
            assert np.array_equal(got.astype(np.float64), ref), c
        elif n == 67:
            for m in K.MUTANTS["skinny"]:
                assert K.ratio(got, K.skinny_ref64(x, w, c["scale"], K.STREAM, c["p"], mutant=m)[0], bound) > 1.0, (m, c)
    print(f"skinny: max err/bound {worst:.3f}")
    assert not bad, bad[:5]


# ---- token reduction ---------------------------------------------------------------------------------------------------------
def _tn_run(l, st, c, t, x, init, gather, det, part):
    """One lr_lora_tn_f32 call. gather: None = 16-byte aligned rows (the LDS-staged kernel), "tcol" / "ldx" = the 2-byte gather
    kernel through a t column offset of 4 / a row stride of cols + 4. Returns the outputs' float32 bits (None: null output)."""
    layout, nj, cols, r, hd, have = K.TN_CONFIGS[c["config"]]
    n = c["n"]
    tcol = 4 if gather == "tcol" else 8
    ldx = cols + 4 if gather == "ldx" else cols + 8
    tb = torch.full((n + 1, 48), POISON, dtype=torch.int16)
    for a in range(nj):
        tb[:n, tcol + 16 * a:tcol + 16 * a + 16] = _bits(t[a])
    tb = tb.cuda()
    xb = _buf(x, ldx)
    outs = [_f32buf(init[a]) if init[a] is not None else None for a in range(2)]
    if det:
        part.fill_(float("nan"))
    _ok(l.lr_lora_tn_f32(nj, tb.data_ptr(), 48, tcol, xb.data_ptr(), ldx, n, cols, c["scale"],
                         outs[0].data_ptr() if outs[0] is not None else None, outs[1].data_ptr() if outs[1] is not None else None,
                         r, layout, hd, K.STREAM, c["p"], part.data_ptr() if det else None, part.numel() - 8 if det else 0, st))
    torch.cuda.synchronize()
    res = []
    for a in range(2):
        if outs[a] is None:
            res.append(None)
            continue
        o = outs[a].cpu().numpy()
        assert (o[-8:] == np.float32(GUARD32)).all(), ("guard floats behind the output written", c)
        res.append(o[:-8].copy())
    if det:
        assert torch.isnan(part[-8:]).all(), ("guard floats behind the partial tiles written", c)
    return res


@pytest.mark.parametrize("config", list(K.TN_CONFIGS))
def test_token_reduction_every_arm(config):
    """Default and deterministic modes, the LDS-staged and the gather kernel: each inside the bound on random operands, all four bit
    for bit on exact ones; the two kernels agree bit for bit wherever the order of additions is fixed; two deterministic runs
    agree; the partial tiles asked for the largest n serve every smaller one."""
    l, st = _L()
    layout, nj, cols, r, hd, have = K.TN_CONFIGS[config]
    n_max = max(c["n"] for c in K.tn_cases() if c["config"] == config)
    part = torch.empty(l.lr_lora_tn_det_floats(nj, n_max, cols, r, layout) + 8, dtype=torch.float32, device="cuda")
    worst, bad, seen = 0.0, [], set()
    for c in (c for c in K.tn_cases() if c["config"] == config):
        t, x, init = K.tn_data(c)
        refs, bounds = K.tn_ref64(t, x, c["scale"], r, layout, hd, K.STREAM, c["p"], init)
        how = c["gather"]
        runs = {(g, d): _tn_run(l, st, c, t, x, init, g, d, part) for g in (None, how) for d in (False, True)}
        again = _tn_run(l, st, c, t, x, init, None, True, part)
        one_chunk = c["n"] <= K.tn_chunk(c["n"])
        for a in range(2):
            assert (refs[a] is None) == (runs[(None, False)][a] is None)
            if refs[a] is None:
                continue
            shape = refs[a].shape
            for key, got in runs.items():
                rr = K.ratio(got[a].reshape(shape), refs[a], bounds[a])
                worst = max(worst, rr)
                if rr > 1.0:
                    bad.append((c, key, a, rr))
                if c["kind"] == "exact":
                    assert np.array_equal(got[a].reshape(shape).astype(np.float64), refs[a]), (c, key, a)
            assert np.array_equal(runs[(None, True)][a].view(np.uint32), runs[(how, True)][a].view(np.uint32)), (c, "kernels differ")
            assert np.array_equal(runs[(None, True)][a].view(np.uint32), again[a].view(np.uint32)), (c, "two deterministic runs")
            if one_chunk:
                assert np.array_equal(runs[(None, False)][a].view(np.uint32), runs[(how, False)][a].view(np.uint32)), c
        if c["kind"] == "random" and c["n"] in (33, 100, 600):
            a = 0 if have[0] else 1
            got = runs[(None, False)][a].reshape(refs[a].shape)
            for m in K.MUTANTS["tn"]:
                chunk = K.tn_chunk(c["n"])
                applies = {"last_partial_step_dropped": (c["n"] % chunk) % 32 != 0, "tail_rows_not_zeroed": c["n"] % 32 != 0,
                           "no_deinterleave": layout == 2, "gate_up_swapped": layout == 3, "assign_not_add": True}[m]
                if applies:
                    mref = K.tn_ref64(t, x, c["scale"], r, layout, hd, K.STREAM, c["p"], init, mutant=m)[0][a]
                    assert K.ratio(got, mref, bounds[a]) > 1.0, (m, c)
                    seen.add(m)
    print(f"token reduction {config}: max err/bound {worst:.3f}; mutants outside: {sorted(seen)}")
    assert not bad, bad[:5]


# ---- expand-add --------------------------------------------------------------------------------------------------------------
def test_expand_within_bound_dropped_elements_keep_their_bits():
    l, st = _L()
    worst, bad = 0.0, []
    for c in K.expand_cases():
        n, cols, r, tcol = c["n"], c["cols"], c["r"], c["tcol"]
        y, t, w = K.expand_data(c)
        yb, tb, wb = _buf(y, cols + 8), _buf(t, 32, col0=tcol), _buf(w, guard_rows=0)
        _ok(l.lr_lora_expand_bf16(yb.data_ptr(), cols + 8, n, cols, tb.data_ptr(), 32, tcol, wb.data_ptr(), r, c["s"], K.STREAM,
                                  c["p"], st))
        torch.cuda.synchronize()
        written = np.zeros((n + 1, cols + 8), bool)
        written[:n, :cols] = True
        assert _poison_kept(yb, written), ("guard row / columns written", c)
        got = _f(yb)[:n, :cols]
        ref, bound = K.expand_ref64(y, t, w, r, c["s"], K.STREAM, c["p"])
        rr = K.ratio(got, ref, bound)
        worst = max(worst, rr)
        if rr > 1.0:
            bad.append((c, rr))
        dropped = ~K.keep(K.STREAM, n, cols, c["p"])
        assert np.array_equal(got[dropped], y[dropped])
        if c["kind"] == "exact":
            assert np.array_equal(got.astype(np.float64), ref), c
        elif n == 9 and cols >= 64:
            for m in K.MUTANTS["expand"]:
                if (m == "mask_of_next_row" and c["p"] == 0.0) or (m == "product_not_rounded" and (c["si"] == 0 or c["cols"] < 2048)):
                    continue
                assert K.ratio(got, K.expand_ref64(y, t, w, r, c["s"], K.STREAM, c["p"], mutant=m)[0], bound) > 1.0, (m, c)
    print(f"expand: max err/bound {worst:.3f}")
    assert not bad, bad[:5]


# ---- SwiGLU ------------------------------------------------------------------------------------------------------------------
def test_swiglu_forward_and_backward_within_bound():
    from tests.test_gpu_stage2_bounds import gated_ratio

    l, st = _L()
    worst_f, worst_b, bad = 0.0, 0.0, []
    for n in K.SWIGLU_NS:
        for f in K.SWIGLU_FS:
            g, u, dy = K.swiglu_data(n, f, seed=n + f)
            gu = K.interleave_gu(g, u)
            gub, dhb = _buf(gu), _buf(dy)
            h = torch.full((n + 1, f), POISON, dtype=torch.int16, device="cuda")
            _ok(l.lr_swiglu_fwd_bf16(gub.data_ptr(), h.data_ptr(), n, f, st))
            torch.cuda.synchronize()
            assert (h[n].cpu().numpy().view(np.uint16) == POISON).all() and np.array_equal(_f(gub)[:n], gu)
            rf = gated_ratio(2, gu.astype(np.float64), np.zeros(gu.shape), 1, _f(h)[:n])
            _ok(l.lr_swiglu_bwd_bf16(gub.data_ptr(), dhb.data_ptr(), n, f, st))
            torch.cuda.synchronize()
            assert (gub[n].cpu().numpy().view(np.uint16) == POISON).all() and np.array_equal(_f(dhb)[:n], dy)
            dg, du = K.deinterleave_gu(_f(gub)[:n])
            rg, ru, bg, bu = K.swiglu_bwd_ref64(g, u, dy)
            rb = max(K.ratio(dg, rg, bg), K.ratio(du, ru, bu))
            print(f"swiglu n={n} f={f}: forward err/bound {rf:.3f}, backward {rb:.3f}")
            worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
            if not (rf <= 1.0 and rb <= 1.0):
                bad.append((n, f, rf, rb))
            if f >= 48:
                for m in K.MUTANTS["swiglu_bwd"]:
                    mg, mu, _, _ = K.swiglu_bwd_ref64(g, u, dy, mutant=m)
                    assert max(K.ratio(dg, mg, bg), K.ratio(du, mu, bu)) > 1.0, (m, n, f)
    print(f"swiglu forward: max err/bound {worst_f:.3f}; swiglu backward: max err/bound {worst_b:.3f}")
    assert not bad, bad


def test_swiglu_over_the_grid_cap_equals_its_row_slices():
    """n f / 8 = 4 205 056 16-byte groups need 16 426 workgroups of 256 against the 16 384-workgroup cap: the threads of the
    first 42 workgroups take a second trip of the grid-stride loop, which covers the last 8 rows. The same kernels on 512-row
    slices (one trip) must give the same bits."""
    l, st = _L()
    n, f = 3056, 11008
    gen = torch.Generator(device="cuda").manual_seed(5)
    gu = (torch.randn(n, 2 * f, generator=gen, device="cuda") * 2).to(torch.bfloat16).view(torch.int16)
    dh = torch.randn(n, f, generator=gen, device="cuda").to(torch.bfloat16).view(torch.int16)
    h = torch.full((n, f), POISON, dtype=torch.int16, device="cuda")
    hs = torch.full((n, f), POISON, dtype=torch.int16, device="cuda")
    _ok(l.lr_swiglu_fwd_bf16(gu.data_ptr(), h.data_ptr(), n, f, st))
    for r0 in range(0, n, 512):
        _ok(l.lr_swiglu_fwd_bf16(gu[r0:].data_ptr(), hs[r0:].data_ptr(), min(512, n - r0), f, st))
    torch.cuda.synchronize()
    assert torch.equal(h, hs) and not (h == POISON).any()
    whole, sliced = gu.clone(), gu.clone()
    _ok(l.lr_swiglu_bwd_bf16(whole.data_ptr(), dh.data_ptr(), n, f, st))
    for r0 in range(0, n, 512):
        _ok(l.lr_swiglu_bwd_bf16(sliced[r0:].data_ptr(), dh[r0:].data_ptr(), min(512, n - r0), f, st))
    torch.cuda.synchronize()
    assert torch.equal(whole, sliced) and not torch.equal(whole, gu)
    # the last rows against float64 (rows of the second trip)
    g, u = K.deinterleave_gu(_f(gu[-2:]))
    dg, du = K.deinterleave_gu(_f(whole[-2:]))
    rg, ru, bg, bu = K.swiglu_bwd_ref64(g, u, _f(dh[-2:]))
    assert max(K.ratio(dg, rg, bg), K.ratio(du, ru, bu)) <= 1.0


# ---- RMSNorm backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", K.NORM_DS)
def test_rmsnorm_backward_every_arm(d):
    l, st = _L()
    worst, bad, seen = 0.0, [], set()
    for c in K.rmsnorm_cases():
        if c["d"] != d:
            continue
        rows, ldt = c["rows"], c["ldt"]
        dy, x, w, res, lora, perm = K.rmsnorm_data(c)
        dyb, xb, wb = _buf(dy, guard_rows=0), _buf(x, guard_rows=0), _buf(w[None], guard_rows=0)
        resb = _buf(res, guard_rows=0) if res is not None else None
        out_n = rows + 3
        out = torch.full((out_n, d), POISON, dtype=torch.int16, device="cuda")
        permb = torch.from_numpy(perm).cuda() if perm is not None else None
        dtb = _buf(lora["dt"], ldt, guard_rows=0) if lora else None
        ab = _buf(lora["a_cat"], guard_rows=0) if lora else None
        _ok(l.lr_rmsnorm_bwd_bf16(dyb.data_ptr(), xb.data_ptr(), wb.data_ptr(), resb.data_ptr() if res is not None else None,
                                  out.data_ptr(), rows, d, 1e-5, permb.data_ptr() if perm is not None else None,
                                  dtb.data_ptr() if lora else None, ldt, ab.data_ptr() if lora else None, c["r"],
                                  lora["stream"] if lora else 0, c["p"] if lora else 0.0, st))
        torch.cuda.synchronize()
        where = perm if perm is not None else np.arange(rows)
        written = np.zeros((out_n, d), bool)
        written[where] = True
        assert _poison_kept(out, written), ("a row that is not listed was written", c)
        assert np.array_equal(_f(dyb), dy) and np.array_equal(_f(xb), x)
        got = _f(out)[where]
        ref, bound = K.rmsnorm_bwd_ref64(dy, x, w, 1e-5, res, lora)
        rr = K.ratio(got, ref, bound)
        worst = max(worst, rr)
        if rr > 1.0:
            bad.append((c, rr))
        if d >= 64:
            for m in K.MUTANTS["rmsnorm_bwd"]:
                applies = {"coef_missing": True, "mean_over_chunks": d % 2048 != 0, "res_before_rounding": c["res"] and rows >= 4,
                           "mask_of_next_row": c["lora"] and c["p"] > 0}[m]
                if applies:
                    assert K.ratio(got, K.rmsnorm_bwd_ref64(dy, x, w, 1e-5, res, lora, mutant=m)[0], bound) > 1.0, (m, c)
                    seen.add(m)
    print(f"rmsnorm backward d={d}: max err/bound {worst:.3f}; mutants outside: {sorted(seen)}")
    assert not bad, bad[:5]


@pytest.mark.parametrize("d", [12, 8200])
def test_rmsnorm_backward_refuses_other_widths_and_writes_nothing(d):
    l, st = _L()
    z = torch.zeros((2, 8208), dtype=torch.int16, device="cuda")
    out = torch.full((2, 8208), POISON, dtype=torch.int16, device="cuda")
    rc = l.lr_rmsnorm_bwd_bf16(z.data_ptr(), z.data_ptr(), z.data_ptr(), None, out.data_ptr(), 2, d, 1e-5, None, None, 32, None, 8,
                               0, 0.0, st)
    torch.cuda.synchronize()
    assert rc == -2 and b"hidden_size" in l.lr_last_error() and bool((out == POISON).all())


# ---- loss head ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", K.CE_VS)
def test_cross_entropy_every_regime(V):
    l, st = _L()
    worst, bad = 0.0, []
    for c in K.ce_cases():
        if c["V"] != V:
            continue
        m = c["m"]
        x, tg = K.ce_data(c["regime"], m, V, c["seed"])
        R = K.ce_ref64(x, tg, K.CE_GSCALE)
        tgb = torch.from_numpy(tg).cuda()
        prev = None
        for det in (0, 1, 1):
            lb = _buf(x)
            scal = torch.full((2 + m + 4,), float("nan"), dtype=torch.float32, device="cuda")
            out = torch.full((3 + 4,), float("nan"), dtype=torch.float32, device="cuda")
            _ok(l.lr_ce_bf16(lb.data_ptr(), m, V, tgb.data_ptr(), K.CE_GSCALE, scal.data_ptr(), out.data_ptr(), det, st))
            torch.cuda.synchronize()
            assert (lb[m].cpu().numpy().view(np.uint16) == POISON).all(), ("guard row written", c)
            assert torch.isnan(out[3:]).all() and torch.isnan(scal[2 + m:]).all() and (det or torch.isnan(scal[2:]).all())
            grad, o = _f(lb)[:m], out[:3].cpu().numpy()
            dead = (tg < 0) | (tg >= V)
            assert not grad[dead].any() and o[1] == m and o[2] == dead.sum()
            rg, ro = K.ratio(grad, R["grad"], R["grad_bound"]), K.ratio(o, R["out"], R["out_bound"])
            worst = max(worst, rg, ro)
            if not (rg <= 1.0 and ro <= 1.0):
                bad.append((c, det, rg, ro))
            if det:
                bits = (lb.cpu().numpy().copy(), out[:3].cpu().numpy().view(np.uint32).copy())
                if prev is not None:
                    assert np.array_equal(prev[0], bits[0]) and np.array_equal(prev[1], bits[1]), ("two deterministic runs", c)
                prev = bits
            if m == 40 and c["regime"] in ("flat", "spike"):
                for mu in K.MUTANTS["ce"]:
                    M = K.ce_ref64(x, tg, K.CE_GSCALE, mutant=mu)
                    assert max(K.ratio(grad, M["grad"], R["grad_bound"]), K.ratio(o, M["out"], R["out_bound"])) > 1.0, (mu, c)
    print(f"cross-entropy V={V}: max err/bound {worst:.3f}")
    assert not bad, bad[:5]


# ---- rowdot ------------------------------------------------------------------------------------------------------------------
def test_rowdot_every_head_dim():
    l, st = _L()
    worst, bad = 0.0, []
    for c in K.rowdot_cases():
        hd, items = c["hd"], c["items"]
        n, nh = {15: (5, 3), 16: (4, 4)}.get(items, (items, 1))
        o, d_o = K.rowdot_data(c)
        ob, db = _buf(o), _buf(d_o)
        out = torch.full((items + 8,), float("nan"), dtype=torch.float32, device="cuda")
        _ok(l.lr_rowdot_bf16(ob.data_ptr(), db.data_ptr(), n, nh, hd, out.data_ptr(), st))
        torch.cuda.synchronize()
        assert torch.isnan(out[items:]).all(), ("guard floats written", c)
        got = out[:items].cpu().numpy()
        ref, bound = K.rowdot_ref64(o, d_o)
        rr = K.ratio(got, ref, bound)
        worst = max(worst, rr)
        if rr > 1.0:
            bad.append((c, rr))
        if c["kind"] == "exact":
            assert np.array_equal(got.astype(np.float64), ref), c
        elif hd == 256:
            assert K.ratio(got, K.rowdot_ref64(o, d_o, mutant="second_step_missing")[0], bound) > 1.0
    print(f"rowdot: max err/bound {worst:.3f}")
    assert not bad, bad[:5]


# ---- AdamW -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.ADAMW_NS)
def test_adamw_clip_steps_and_both_norms(n):
    l, st = _L()
    worst, bad, seen = 0.0, [], set()
    for c in K.adamw_cases():
        if c["n"] != n:
            continue
        p, g, m, v = K.adamw_data(n, c["seed"])
        limit = K.adamw_limit(c, g)
        R = K.adamw_ref64(p, g, m, v, c["step"], limit=limit, wd=c["wd"], **K.ADAMW_HYPER)
        norms = []
        for det in (0, 1, 1):
            pb, gb, mb, vb = (_f32buf(a) for a in (p, g, m, v))
            scratch = torch.full((4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
            ctr = torch.tensor([c["step"] - 1, 777], dtype=torch.int32, device="cuda")
            norm = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
            h = K.ADAMW_HYPER
            _ok(l.lr_lora_adamw_f32(pb.data_ptr(), gb.data_ptr(), mb.data_ptr(), vb.data_ptr(), n, scratch.data_ptr(), ctr.data_ptr(),
                                    h["lr"], limit, h["beta1"], h["beta2"], h["eps"], c["wd"], norm.data_ptr(), det, st))
            torch.cuda.synchronize()
            assert ctr.tolist() == [c["step"], 777], "the step counter moves by exactly one"
            assert torch.isnan(scratch[4:]).all() and torch.isnan(norm[1:]).all()
            got = {k: b.cpu().numpy() for k, b in (("p", pb), ("m", mb), ("v", vb), ("g", gb))}
            for k in got:
                assert (got[k][n:] == np.float32(GUARD32)).all(), ("guard floats written", k, c)
            assert np.array_equal(got["g"][:n].view(np.uint32), g.view(np.uint32)), "the gradient is read only"
            nv = norm[:1].cpu().numpy()
            ratios = [K.ratio(got[k][:n], R[k], R[k + "_bound"]) for k in ("p", "m", "v")] + [K.ratio(nv, R["norm"], R["norm_bound"])]
            worst = max(worst, *ratios)
            if max(ratios) > 1.0:
                bad.append((c, det, ratios))
            if det:
                norms.append(nv.view(np.uint32)[0])
            for mu in K.MUTANTS["adamw"]:
                if (mu == "no_clip" and c["clip"] != "active") or (mu == "bias_step_minus_one" and c["step"] == 1):
                    continue
                M = K.adamw_ref64(p, g, m, v, c["step"], limit=limit, wd=c["wd"], mutant=mu, **h)
                assert max(K.ratio(got["p"][:n], M["p"], R["p_bound"]), K.ratio(got["m"][:n], M["m"], R["m_bound"])) > 1.0, (mu, c)
                seen.add(mu)
        assert norms[0] == norms[1], ("two deterministic norms", c)
    print(f"AdamW n={n}: max err/bound {worst:.3f}; mutants outside: {sorted(seen)}")
    assert not bad, bad[:5]


# ---- forward sweep and rotation backward -------------------------------------------------------------------------------------
_TABLES = {}


def _table(hd):
    """lr_rope_table for ROPE_T positions: (device table, cos, sin as read back [T][hd / 2]), made once per head size."""
    if hd not in _TABLES:
        from llamarec_amd._lib import check

        l, st = _L()
        cs = torch.full((l.lr_rope_table_bytes(K.ROPE_T, hd) // 4,), float("nan"), dtype=torch.float32, device="cuda")
        check(l.lr_rope_table(cs.data_ptr(), K.ROPE_T, hd, 10000.0, st), "rope table")
        torch.cuda.synchronize()
        f = cs[: K.ROPE_T * hd].view(K.ROPE_T, hd // 2, 2).cpu().numpy()
        _TABLES[hd] = (cs, f[..., 0].copy(), f[..., 1].copy())
    return _TABLES[hd]


def _rope_fwd(l, st, c, qkv, t, bq_t, bv_t, tk, bk_t, norm, pos, cs, want_rc=0):
    n, nq, nk, hd = c["n"], c["nq"], c["nk"], c["hd"]
    qw, qk = (nq + 2 * nk) * hd, (nq + nk) * hd
    qb, tb = _buf(qkv), _buf(t, guard_rows=0)
    bqb, bvb = _buf(bq_t, guard_rows=0), _buf(bv_t, guard_rows=0)
    tkb = _buf(tk, 24, guard_rows=0, col0=8) if tk is not None else None
    bkb = _buf(bk_t, guard_rows=0) if bk_t is not None else None
    wqb = _buf(norm["wq"][None], guard_rows=0) if norm else None
    wkb = _buf(norm["wk"][None], guard_rows=0) if norm else None
    xs = torch.full((n + 1, qk), POISON, dtype=torch.int16, device="cuda") if norm else None
    posb = torch.from_numpy(pos).cuda()
    rc = l.lr_lora_rope_fwd_bf16(qb.data_ptr(), n, qw, nq * hd, nk * hd, hd, tb.data_ptr(), bqb.data_ptr(), bvb.data_ptr(), c["r"],
                                 c["s"], posb.data_ptr(), cs.data_ptr(), tkb.data_ptr() if tk is not None else None, 24, 8,
                                 bkb.data_ptr() if bk_t is not None else None, wqb.data_ptr() if norm else None,
                                 wkb.data_ptr() if norm else None, norm["eps"] if norm else 0.0, xs.data_ptr() if norm else None, st)
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, l.lr_last_error())
    assert (qb[n].cpu().numpy().view(np.uint16) == POISON).all(), ("guard row written", c)
    if norm:
        assert (xs[n].cpu().numpy().view(np.uint16) == POISON).all(), ("guard row of the save buffer written", c)
    return _f(qb)[:n], (_f(xs)[:n] if norm else None)


@pytest.mark.parametrize("nq,nk,hd", K.ROPE_SHAPES)
def test_forward_sweep_all_four_instantiations(nq, nk, hd):
    l, st = _L()
    cs, cos, sin = _table(hd)
    worst, bad, seen = 0.0, [], set()
    for c in K.rope_fwd_cases():
        if (c["nq"], c["nk"], c["hd"]) != (nq, nk, hd):
            continue
        n, r, s = c["n"], c["r"], c["s"]
        pos = K.rope_positions(n)
        qkv, t, bq_t, bv_t, tk, bk_t, norm = K.rope_fwd_data(c)
        ref, bound, xs, xsb = K.rope_fwd_ref64(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk, bk_t, norm)
        got, gxs = _rope_fwd(l, st, c, qkv, t, bq_t, bv_t, tk, bk_t, norm, pos, cs)
        rr = K.ratio(got, ref, bound)
        if norm:
            rr = max(rr, K.ratio(gxs, xs, xsb))      # the pre-norm values, exactly (but for a flip the delta's fp32 sum allows)
        worst = max(worst, rr)
        if rr > 1.0:
            bad.append((c, rr))
        if norm and not c["hask"]:
            assert np.array_equal(gxs[:, nq * hd:], qkv[:, nq * hd:(nq + nk) * hd]), "k without an adapter is saved as it came"
        if n == 9:
            for m in K.MUTANTS["rope_fwd"]:
                if m == "norm_before_delta" and not norm:
                    continue
                mref = K.rope_fwd_ref64(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk, bk_t, norm, mutant=m)[0]
                assert K.ratio(got, mref, bound) > 1.0, (m, c)
                seen.add(m)
    print(f"forward sweep nq={nq} nk={nk} hd={hd}: max err/bound {worst:.3f}; mutants outside: {sorted(seen)}")
    assert not bad, bad[:5]


def test_forward_sweep_with_a_norm_refuses_head_dim_96_and_writes_nothing():
    l, st = _L()
    c = dict(n=5, nq=2, nk=2, hd=96, hask=False, norm=True, r=8, s=4.0, kind="random", seed=3)
    cs, _, _ = _table(96)
    qkv, t, bq_t, bv_t, tk, bk_t, norm = K.rope_fwd_data(c)
    got, gxs = _rope_fwd(l, st, c, qkv, t, bq_t, bv_t, tk, bk_t, norm, K.rope_positions(5), cs, want_rc=-2)
    assert b"head_dim 96" in l.lr_last_error() and np.array_equal(got, qkv) and np.isnan(gxs).all()


def _rope_bwd(l, st, x, n, qw, rot, hd, posb, cs):
    xb = _buf(x)
    _ok(l.lr_rope_bwd_bf16(xb.data_ptr(), n, qw, rot, hd, posb.data_ptr(), cs.data_ptr(), st))
    torch.cuda.synchronize()
    assert (xb[n].cpu().numpy().view(np.uint16) == POISON).all()
    return _f(xb)[:n]


@pytest.mark.parametrize("nq,nk,hd", K.ROPE_SHAPES)
def test_rotation_backward_bits_bound_and_adjoint_identity(nq, nk, hd):
    l, st = _L()
    cs, cos, sin = _table(hd)
    heads, qw, rot = nq + nk, (nq + 2 * nk) * hd, (nq + nk) * hd
    for n in (1, 5, 9):
        pos = K.rope_positions(n)
        posb = torch.from_numpy(pos).cuda()
        y = K.operands("random", 70 + n + hd, (n, qw))
        got = _rope_bwd(l, st, y, n, qw, rot, hd, posb, cs)
        assert np.array_equal(got[:, rot:], y[:, rot:]), "the v columns are not rotated"
        ref, bound = K.rope_bwd_ref64(y[:, :rot], heads, hd, pos, cos, sin)
        rr = K.ratio(got[:, :rot], ref, bound)
        print(f"rotation backward nq={nq} nk={nk} hd={hd} n={n}: err/bound {rr:.3f}")
        assert rr <= 1.0
        assert np.array_equal(got[:, :rot], K.rope_bwd_emul32(y[:, :rot], heads, hd, pos, cos, sin)), "two products, a sum, one rounding"
        assert K.ratio(got[:, :rot], K.rope_bwd_ref64(y[:, :rot], heads, hd, pos, cos, sin, "forward_rotation")[0], bound) > 1.0
        # <R x, y> = <x, R^T y> with R x from the forward sweep under zero adapters
        c = dict(n=n, nq=nq, nk=nk, hd=hd, hask=False, norm=False, r=4, s=1.0, kind="exact", seed=n)
        x = K.operands("random", 80 + n + hd, (n, qw))
        z16, z32 = np.zeros((16, 1), np.float32), np.zeros((n, 32), np.float32)
        rx, _ = _rope_fwd(l, st, c, x, z32, z16 + np.zeros((16, nq * hd), np.float32), z16 + np.zeros((16, nk * hd), np.float32),
                          None, None, None, pos, cs)
        assert np.array_equal(rx[:, rot:], x[:, rot:])
        fref, fbound, _, _ = K.rope_fwd_ref64(x, nq, nk, hd, z32, np.zeros((16, nq * hd)), np.zeros((16, nk * hd)), 4, 1.0, pos, cos, sin)
        lhs, rhs = (rx[:, :rot].astype(np.float64) * y[:, :rot]).sum(), (x[:, :rot].astype(np.float64) * got[:, :rot]).sum()
        tol = (fbound[:, :rot] * np.abs(y[:, :rot])).sum() + (np.abs(x[:, :rot]) * bound).sum()
        assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


def test_rotation_backward_over_the_grid_cap_equals_its_row_slices():
    """2064 rows of 8192 rotated columns are 8256 workgroups' worth against the 8192-workgroup cap: some threads take a second trip of
    the grid-stride loop. The same kernel on 512-row slices must give the same bits; first, last and 64 sampled rows against float64."""
    l, st = _L()
    n, qw, hd = 2064, 8192, 128
    cs, cos, sin = _table(hd)
    gen = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(n, qw, generator=gen, device="cuda").to(torch.bfloat16).view(torch.int16)
    pos = ((np.arange(n, dtype=np.int64) * 40503) % K.ROPE_T).astype(np.int32)
    posb = torch.from_numpy(pos).cuda()
    whole, sliced = x.clone(), x.clone()
    _ok(l.lr_rope_bwd_bf16(whole.data_ptr(), n, qw, qw, hd, posb.data_ptr(), cs.data_ptr(), st))
    for r0 in range(0, n, 512):
        _ok(l.lr_rope_bwd_bf16(sliced[r0:].data_ptr(), min(512, n - r0), qw, qw, hd, posb[r0:].data_ptr(), cs.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(whole, sliced) and not torch.equal(whole, x)
    rows = np.unique(np.r_[0, n - 1, (np.arange(64) * 2654435761) % n])
    ridx = torch.from_numpy(rows).cuda()
    ref, bound = K.rope_bwd_ref64(_f(x[ridx]), qw // hd, hd, pos[rows], cos, sin)
    rr = K.ratio(_f(whole[ridx]), ref, bound)
    print(f"rotation backward over the cap: err/bound {rr:.3f}")
    assert rr <= 1.0


# ---- SwiGLU with the gate / up adapters --------------------------------------------------------------------------------------
def test_swiglu_with_adapters_writes_the_sum_back():
    from tests.test_gpu_stage2_bounds import gated_ratio

    l, st = _L()
    worst, bad = 0.0, []
    for a, n in enumerate(K.SWIGLU_NS):
        for b, f in enumerate(K.SWIGLU_FS):
            r, s = (4, 8, 16)[(a + b) % 3], (4.0, 1.4285714)[(a + b // 2) % 2]     # each r and each scale meet each n and each f
            g, u, t, w = K.swiglu_lora_data(n, f, r, seed=n + f + r)
            gu = K.interleave_gu(g, u)
            gub, tb, wb = _buf(gu), _buf(t, 40, guard_rows=0, col0=8), _buf(w, guard_rows=0)
            h = torch.full((n + 1, f), POISON, dtype=torch.int16, device="cuda")
            _ok(l.lr_swiglu_lora_fwd_bf16(gub.data_ptr(), h.data_ptr(), n, f, tb.data_ptr(), 40, 8, wb.data_ptr(), r, s, st))
            torch.cuda.synchronize()
            assert (h[n].cpu().numpy().view(np.uint16) == POISON).all() and (gub[n].cpu().numpy().view(np.uint16) == POISON).all()
            g1, u1, Dg, Du = K.swiglu_lora_ref64(g, u, t, w, r, s)
            gg, gu_ = K.deinterleave_gu(_f(gub)[:n])
            r_gu = max(K.ratio(gg, g1, Dg + K.TINY), K.ratio(gu_, u1, Du + K.TINY))
            D = K.interleave_gu(Dg.astype(np.float32), Du.astype(np.float32)).astype(np.float64)
            gu1 = K.interleave_gu(g1.astype(np.float32), u1.astype(np.float32)).astype(np.float64)
            r_h = gated_ratio(2, gu1, D * 2.0 ** 24, 1, _f(h)[:n])
            print(f"swiglu with adapters n={n} f={f} r={r}: gate/up err/bound {r_gu:.3f}, h {r_h:.3f}")
            worst = max(worst, r_gu, r_h)
            if not (r_gu <= 1.0 and r_h <= 1.0):
                bad.append((n, f, r, r_gu, r_h))
            mg, mu, _, _ = K.swiglu_lora_ref64(g, u, t, w, r, s, mutant="gate_up_ranks_swapped")
            assert max(K.ratio(gg, mg, Dg + K.TINY), K.ratio(gu_, mu, Du + K.TINY)) > 1.0
    print(f"swiglu with adapters: max err/bound {worst:.3f}")
    assert not bad, bad


# ---- working copies and the transpose: bit-exact -----------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 96, 128])
def test_working_copies_bit_exact(hd):
    l, st = _L()
    d, qcols, vcols, f = 40, 2 * hd, hd, 48
    for r in (1, 8, 16):
        aq, av = K.hash_uniform(r + hd, (r, d), 0.1), K.hash_uniform(r + hd + 1, (r, d), 0.1)
        bq, bv = K.hash_uniform(r + hd + 2, (qcols, r), 0.1), K.hash_uniform(r + hd + 3, (vcols, r), 0.1)
        dev = [torch.from_numpy(a).cuda() for a in (aq, bq, av, bv)]
        a_cat = torch.full((32 + 1, d), POISON, dtype=torch.int16, device="cuda")
        bq_t = torch.full((16 + 1, qcols), POISON, dtype=torch.int16, device="cuda")
        bv_t = torch.full((16 + 1, vcols), POISON, dtype=torch.int16, device="cuda")
        _ok(l.lr_lora_prep_bf16(*(t.data_ptr() for t in dev), r, d, qcols, vcols, hd, a_cat.data_ptr(), bq_t.data_ptr(),
                                bv_t.data_ptr(), st))
        torch.cuda.synchronize()
        want = K.prep_lora_ref(aq, bq, av, bv, r, hd)
        for got, w, rows in ((a_cat, want[0], 32), (bq_t, want[1], 16), (bv_t, want[2], 16)):
            assert (got[rows].cpu().numpy().view(np.uint16) == POISON).all(), "guard row written"
            assert np.array_equal(got[:rows].cpu().numpy().view(np.uint16), f32_to_bf16_bits(w)), (r, hd)
        for perm in (0, 1, 2, 3):
            out = f if perm >= 2 else qcols
            ldb = 2 * out + 8 if perm >= 2 else out + 8
            a, b = K.hash_uniform(perm + r, (r, d), 0.1), K.hash_uniform(perm + r + 9, (out, r), 0.1)
            a_w = torch.full((16 + 1, d), POISON, dtype=torch.int16, device="cuda")
            b_t = torch.full((16 + 1, ldb), POISON, dtype=torch.int16, device="cuda")
            ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            _ok(l.lr_lora_prep_module_bf16(ad.data_ptr(), bd.data_ptr(), r, d, out, perm, hd, a_w.data_ptr(), b_t.data_ptr(), ldb, st))
            torch.cuda.synchronize()
            before = bf16_bits_to_f32(np.full((16, ldb), POISON, np.uint16))
            wa, wb = K.prep_module_ref(a, b, r, perm, hd, before)
            assert np.array_equal(a_w[:16].cpu().numpy().view(np.uint16), f32_to_bf16_bits(wa))
            # the other half of the gate / up pair, the columns past `out` and the guard rows keep the bits they had
            assert np.array_equal(b_t[:16].cpu().numpy().view(np.uint16), f32_to_bf16_bits(wb).astype(np.uint16)), (r, hd, perm)
            assert (b_t[16].cpu().numpy().view(np.uint16) == POISON).all() and (a_w[16].cpu().numpy().view(np.uint16) == POISON).all()


@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (64, 64), (130, 200)])
def test_transpose_bit_exact(rows, cols):
    l, st = _L()
    src = (torch.arange(rows * cols, dtype=torch.int32) * 40503 % 65521).to(torch.int16).view(rows, cols).cuda()
    dst = torch.full((cols * rows + 16,), POISON, dtype=torch.int16, device="cuda")
    _ok(l.lr_transpose_bf16(src.data_ptr(), rows, cols, dst.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(dst[: rows * cols].view(cols, rows), src.t()) and bool((dst[rows * cols:] == POISON).all())
