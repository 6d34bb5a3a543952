"""GPU: the retriever step's item GEMM + softmax cross-entropy alone (lr_lru_train_ce_parity), in its three forms -- stored logits
on row panels (csrc/lru_train_scores.hip), fused (csrc/lru_train_ce.hip), generic GEMM launches around tr_ce_kernel -- against
the float64 reference of tests/lru_train_ref.py, element by element within the bounds derived there, at the shapes where the
launchers' splits change (asserted through lr_lru_train_ce_plan). Gradient buffers carry guard rows of a sentinel bit pattern
that must survive, rows without a usable label must come back as exact zeros, and every case prints max(err / bound) and shows
that one named mutant of the reference exceeds the bound on the same data."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import lru_train_ref as KR

pytestmark = pytest.mark.gpu

SEED = 20                       # tests/test_lru_train_ref_host.py pins the reference on the same data
SENTINEL = 0x7FC12345           # a NaN with a payload
FORMS = (0, 1, 2)
# what each shape reaches: {form: the leading values of lr_lru_train_ce_plan}
#   form 0: item splits of the score pass, of the d x pass, row parts of the d E pass, 64-item super-blocks, rows padded to 16
#   form 1: item chunks, 32-item tiles per chunk, row chunks of the d E pass, 32-row tiles per chunk
REACHES = {
    (1, 2): {0: [1, 1, 1, 1, 16], 1: [1, 1, 1, 1]},              # smallest legal problem: Rpad = 16, one super-block
    (21, 64): {0: [1, 1, 1, 1, 32], 1: [1, 2, 1, 1]},            # ns = 1; ragged second panel
    (21, 65): {0: [2, 2, 1, 2, 32], 1: [1, 3, 1, 1]},            # one item in a new super-block: ns = ns2 = 2, 63 padded columns
    (84, 121): {0: [2, 2, 1, 2, 96], 1: [1, 4, 1, 3]},           # the golden shape
    (1000, 2081): {0: [32, 8, 7, 33, 1008], 1: [2, 33, 1, 32]},  # ns = 32 of nsb = 33, ns2 = 8, nq > 1, R % 16 = 8; two item chunks (66 tiles)
    (2081, 2081): {0: [23, 7, 7, 33, 2096], 1: [2, 33, 2, 33]},  # two row chunks in pass C; nq = 7 (8 parts would need two rounds of 264 workgroups); bad labels
    (130, 4097): {0: [32, 8, 1, 65, 144], 1: [4, 33, 1, 5]},     # one item past 4096; four item chunks
}
# the mutant each shape shows on its own data (one that applies there in every regime the shape runs)
SHOWN = {(1, 2): "last_tile_missing_from_dE", (21, 64): "ragged_panel_rows_missing", (21, 65): "partials_not_rescaled",
         (84, 121): "onehot_at_label_minus_one", (1000, 2081): "partials_not_rescaled", (2081, 2081): "n_counts_bad_labels",
         (130, 4097): "last_tile_missing_from_dE"}


def plan(form, R, C):
    from llamarec_amd import _lib

    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().lr_lru_train_ce_plan(form, R, C, out), "lr_lru_train_ce_plan")
    return [int(v) for v in out]


@functools.lru_cache(maxsize=4)
def reference(regime, R, C, bad, all_ignored=False):
    """Data, float64 reference and each form's bounds, computed once and shared by the forms (read-only)."""
    x, E, bias, lab = KR.ce_data(regime, R, C, SEED, bad)
    if all_ignored:
        lab = np.zeros_like(lab)
    x64, E64, b64 = (a.astype(np.float64) for a in (x, E, bias))
    ref = KR.ce_ref64(x64, E64, b64, lab)
    plans = {f: plan(f, R, C) for f in FORMS}
    return (x, E, bias, lab), ref, plans


@functools.lru_cache(maxsize=8)
def bounds(regime, R, C, bad, form):
    (x, E, bias, lab), _, plans = reference(regime, R, C, bad)
    return KR.ce_bounds(x.astype(np.float64), E.astype(np.float64), bias.astype(np.float64), lab,
                        KR.chains(form, R, C, plans[form], lab))


def guarded(rows, cols, guard_rows, fill=None):
    """float32 device buffer [rows + guard_rows][cols]: `fill` (or zeros) in front, the sentinel's bits behind."""
    b = torch.full((rows + guard_rows, cols), SENTINEL, dtype=torch.int32)
    b[:rows] = torch.from_numpy(np.zeros((rows, cols), np.float32) if fill is None
                                else np.ascontiguousarray(fill, dtype=np.float32).reshape(rows, cols)).view(torch.int32)
    return b.cuda()


def run(form, x, E, bias, lab, base_dE=None, base_db=None):
    """-> (out_scal[4], dX [R][64], dE [C][64], dbias [C]) float32 numpy; asserts that every guard kept its bits."""
    from llamarec_amd._lib import lib, stream_ptr

    l, R, C = lib(), x.shape[0], E.shape[0]
    xd, Ed, bd, ld = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, E, bias, lab.astype(np.int64)))
    dX = guarded(R, 64, 16)
    dX[:R] = SENTINEL                       # the call zeroes d x itself
    dE, db = guarded(C, 64, 64, base_dE), guarded(C, 1, 64, base_db)
    n_ws = l.lr_lru_train_ce_parity_workspace_bytes(form, R, C)
    assert n_ws > 0
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
    scal = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    rc = l.lr_lru_train_ce_parity(form, xd.data_ptr(), Ed.data_ptr(), bd.data_ptr(), ld.data_ptr(), R, C, ws.data_ptr(), n_ws,
                                  scal.data_ptr(), dX.data_ptr(), dE.data_ptr(), db.data_ptr(), stream_ptr())
    assert rc == 0, (rc, l.lr_last_error())
    torch.cuda.synchronize()
    for name, buf, rows in (("dX", dX, R), ("dE", dE, C), ("dbias", db, C)):
        assert bool((buf[rows:] == SENTINEL).all()), f"{name}: guard rows written"
    f = lambda t, rows: t[:rows].view(torch.float32).cpu().numpy()
    return scal.cpu().numpy(), f(dX, R), f(dE, C), f(db, C).reshape(-1)


def ratios(scal, dX, dE, db, ref, bnd):
    return {"loss": abs(float(scal[0]) - ref[0]) / bnd["loss"], "dX": KR.ratio(dX, ref[2], bnd["dX"]),
            "dE": KR.ratio(dE, ref[3], bnd["dE"]), "dbias": KR.ratio(db, ref[4], bnd["dbias"])}


def test_plans_reach_what_the_table_says():
    for (R, C), want in REACHES.items():
        for form, w in want.items():
            assert plan(form, R, C)[:len(w)] == w, (R, C, form, plan(form, R, C))
    assert REACHES[(1000, 2081)][0][2] > 1 and REACHES[(1000, 2081)][1][0] * REACHES[(1000, 2081)][1][1] == 66


# every shape for all three forms and all four regimes (forms innermost: they share one reference); `shifted` is left out where C
# is a multiple of 64: no padded column there, the regime would repeat `flat` with another bias
CASES = [(R, C, bad, regime, form) for R, C, bad in KR.SHAPES for regime in KR.REGIMES for form in FORMS
         if not (regime == "shifted" and C % 64 == 0)]


@pytest.mark.parametrize("R,C,bad,regime,form", CASES)
def test_cross_entropy_within_bound(R, C, bad, regime, form):
    (x, E, bias, lab), ref, plans = reference(regime, R, C, bad)
    if form in REACHES[(R, C)]:
        w = REACHES[(R, C)][form]
        assert plans[form][:len(w)] == w
    bnd = bounds(regime, R, C, bad, form)
    scal, dX, dE, db = run(form, x, E, bias, lab)
    r = ratios(scal, dX, dE, db, ref, bnd)
    print(f"form {form} {regime} R={R} C={C}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    valid = (lab > 0) & (lab < C)
    assert scal[1] == valid.sum() == ref[1] and scal[3] == ((lab < 0) | (lab >= C)).sum()
    assert np.array_equal(dX[~valid], np.zeros_like(dX[~valid])), "rows without a usable label: d x must be exactly zero"
    assert max(r.values()) <= 1.0, r
    # one named mutant of the reference, on this data, is outside this form's bound
    mutant = SHOWN[(R, C)]
    ok, why = KR.mutant_applies(mutant, (x, E, bias, lab), plans)
    assert ok, (mutant, why)
    mut = KR.ce_ref64(x.astype(np.float64), E.astype(np.float64), bias.astype(np.float64), lab, mutant=mutant,
                      splits=max(plans[0][0], plans[1][0]))
    rm = max(ratios([mut[0]], mut[2], mut[3], mut[4], ref, bnd).values())
    print(f"  reference mutant '{mutant}': {rm:.3g} x bound")
    assert rm > 1.0, (mutant, rm)


@pytest.mark.parametrize("form", FORMS)
def test_gradient_buffers_are_added_into(form):
    """d E and d bias start from a random base: result - base is the reference within bound + eps |result| (the base's own
    rounding into the sum)."""
    R, C, bad = 84, 121, False
    (x, E, bias, lab), ref, plans = reference("flat", R, C, bad)
    from llamarec_amd.synth import hash_uniform

    base_E, base_b = hash_uniform(91, (C, 64), 1.0), hash_uniform(92, (C,), 1.0)
    bnd = KR.ce_bounds(x.astype(np.float64), E.astype(np.float64), bias.astype(np.float64), lab,
                       KR.chains(form, R, C, plans[form], lab), base_dE=base_E, base_dbias=base_b)
    scal, dX, dE, db = run(form, x, E, bias, lab, base_E, base_b)
    for name, got, base, want in (("dE", dE, base_E, ref[3]), ("dbias", db, base_b, ref[4])):
        got64 = got.astype(np.float64)
        r = KR.ratio(got64 - base, want, bnd[name] + KR.EPS * np.abs(got64))
        print(f"form {form} {name} over a base: max err / bound {r:.3f}")
        assert r <= 1.0, (name, r)
    assert KR.ratio(dX, ref[2], bnd["dX"]) <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_all_labels_ignored_gives_exact_zeros(form):
    R, C = 21, 65
    (x, E, bias, lab), ref, _ = reference("flat", R, C, False, True)
    scal, dX, dE, db = run(form, x, E, bias, lab)
    assert scal[0] == 0.0 and scal[1] == 0.0 and scal[3] == 0.0     # (the engine's 0 / 0 mean is not this test's business)
    for g in (dX, dE, db):
        assert np.array_equal(g, np.zeros_like(g))


@pytest.mark.parametrize("form", FORMS)
def test_logits_far_below_a_padded_columns_zero(form):
    """Every bias at -100, so every real logit lies about 100 below the 0 a padded column of the stored logits holds, and
    log2(n sum exp) is below -128. The softmax does not care about the shift. Form 0 forms 2^(logit2 - lse2) on the padded columns
    as well, against table fragments that are 0 there: the value has to stay finite, or the d x product adds inf x 0."""
    R, C = 21, 65
    x, E, bias, lab = KR.ce_data("shifted", R, C, SEED)
    bias = np.full(C, -100.0, np.float32)
    x64, E64, b64 = (a.astype(np.float64) for a in (x, E, bias))
    ref = KR.ce_ref64(x64, E64, b64, lab)
    bnd = KR.ce_bounds(x64, E64, b64, lab, KR.chains(form, R, C, plan(form, R, C), lab))
    scal, dX, dE, db = run(form, x, E, bias, lab)
    r = ratios(scal, dX, dE, db, ref, bnd)
    print(f"form {form} bias -100 R={R} C={C}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
