"""CPU: tests/lru_train_ref.py pinned without a GPU. Its float64 reference is the oracle's cross-entropy, its fp32 emulation lies
inside every bound and every mutant outside, on the data tests/test_gpu_lru_train_ce_bounds.py gives the HIP kernels."""
import ctypes
import functools

import numpy as np
import pytest

from tests import lru_train_ref as KR

SEED = 20


def plan(form, R, C):
    """lr_lru_train_ce_plan: host arithmetic of the launchers, no GPU."""
    from llamarec_amd import _lib

    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().lr_lru_train_ce_plan(form, R, C, out), "lr_lru_train_ce_plan")
    return [int(v) for v in out]


@functools.lru_cache(maxsize=None)
def case(regime, R, C, bad):
    x, E, bias, lab = KR.ce_data(regime, R, C, SEED, bad)
    x64, E64, b64 = (a.astype(np.float64) for a in (x, E, bias))
    plans = {f: plan(f, R, C) for f in (0, 1, 2)}
    ref = KR.ce_ref64(x64, E64, b64, lab)
    bounds = {f: KR.ce_bounds(x64, E64, b64, lab, KR.chains(f, R, C, plans[f], lab)) for f in (0, 1, 2)}
    return (x, E, bias, lab), plans, ref, bounds


def ratios(got, ref, bnd):
    return {"loss": abs(got[0] - ref[0]) / bnd["loss"], "dX": KR.ratio(got[2], ref[2], bnd["dX"]),
            "dE": KR.ratio(got[3], ref[3], bnd["dE"]), "dbias": KR.ratio(got[4], ref[4], bnd["dbias"])}


def test_reference_is_the_oracles_cross_entropy(golden_dir, monkeypatch):
    """ce_ref64 on the oracle's own final hidden states (the output of its last forward LayerNorm, caught as it passes)
    reproduces the oracle's loss, d bias and the cross-entropy part of d table (the rest of d table is the embedding lookup's
    scatter of the first LayerNorm's input gradient, caught the same way) to 1e-12 relative."""
    from oracle import lru_train_oracle as TO

    z = np.load(f"{golden_dir}/lru_train_v120.npz", allow_pickle=False)
    names = [str(n) for n in z["param_names"]]
    init = {n: z["init/" + n] for n in names}
    fwd, bwd = [], []
    ln_fwd, ln_bwd = TO._ln_fwd, TO._ln_bwd
    monkeypatch.setattr(TO, "_ln_fwd", lambda *a: (fwd.append(ln_fwd(*a)), fwd[-1])[1])
    monkeypatch.setattr(TO, "_ln_bwd", lambda *a: (bwd.append(ln_bwd(*a)), bwd[-1])[1])
    tok, lab = z["tokens"], z["labels"]
    o_loss, G = TO.loss_and_grads(init, tok, lab)
    x = fwd[-1][0].reshape(-1, 64)
    E, bias = init["embedding.token.weight"].astype(np.float64), init["model.bias"].astype(np.float64)
    loss, n, dX, dE, db = KR.ce_ref64(x, E, bias, lab.reshape(-1))
    assert n == int((lab != 0).sum()) == 55
    assert abs(loss / n - o_loss) <= 1e-12 * abs(o_loss)
    assert np.abs(db - G["model.bias"]).max() <= 1e-12 * np.abs(G["model.bias"]).max()
    lookup = np.zeros_like(E)
    np.add.at(lookup, tok.reshape(-1), bwd[-1][0].reshape(-1, 64))
    ce_part = G["embedding.token.weight"] - lookup
    assert np.abs(dE - ce_part).max() <= 1e-12 * np.abs(ce_part).max()
    assert np.abs(dE).max() > 1e-3 and np.abs(dX).max() > 1e-4


@pytest.mark.parametrize("regime", KR.REGIMES)
@pytest.mark.parametrize("R,C,bad", KR.SHAPES)
def test_emulation_is_inside_every_bound(regime, R, C, bad):
    (x, E, bias, lab), plans, ref, bounds = case(regime, R, C, bad)
    for form, (splits, parts) in {0: (plans[0][1], 4 * plans[0][2]), 1: (plans[1][0], plans[1][2]), 2: (1, 1)}.items():
        order = "fwd" if form != 1 else "rev"
        got = KR.ce_emul32(x, E, bias, lab, item_splits=splits, row_parts=min(parts, R), order=order)
        assert got[1] == ref[1]
        r = ratios(got, ref, bounds[form])
        print(f"emulation {regime} R={R} C={C} form {form}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, (form, r)


@pytest.mark.parametrize("regime", KR.REGIMES)
@pytest.mark.parametrize("R,C,bad", KR.SHAPES)
def test_every_mutant_is_outside_the_bound(regime, R, C, bad):
    """A condition, not a measurement: at every shape where a mutant applies it exceeds the LOOSEST of the three forms' bounds
    on at least one output; where it cannot apply the reason is printed by name."""
    (x, E, bias, lab), plans, ref, bounds = case(regime, R, C, bad)
    x64, E64, b64 = (a.astype(np.float64) for a in (x, E, bias))
    for mutant in KR.MUTANTS:
        ok, why = KR.mutant_applies(mutant, (x, E, bias, lab), plans)
        if not ok:
            print(f"mutant {mutant} not applicable at {regime} R={R} C={C}: {why}")
            continue
        splits = max(plans[0][0], plans[1][0])
        got = KR.ce_ref64(x64, E64, b64, lab, mutant=mutant, splits=splits)
        worst = min(max(ratios(got, ref, bounds[f]).values()) for f in (0, 1, 2))
        print(f"mutant {mutant} {regime} R={R} C={C}: {worst:.3g} x the bound")
        assert worst > 1.0, (mutant, worst)


def test_not_applicable_mutants_are_the_expected_ones():
    """The (shape, mutant) pairs that cannot apply, by name: nothing else is ever left out. The padded column is also out where
    the data puts every labelled row's lse far above a padded column's 0 (peaked: the label's logit is 20 up; wide: the largest of
    many logits of standard deviation 13) -- which is why the shifted regime exists; flat and shifted leave out nothing more."""
    bad_only = "n_counts_bad_labels"
    want = {
        (1, 2): {"partials_not_rescaled", bad_only},
        (21, 64): {"padded_column_counted", "partials_not_rescaled", bad_only},
        (21, 65): {bad_only},
        (84, 121): {bad_only},
        (1000, 2081): {bad_only},
        (2081, 2081): set(),
        (130, 4097): {bad_only},
    }
    for R, C, bad in KR.SHAPES:
        plans = {f: plan(f, R, C) for f in (0, 1, 2)}
        for regime in KR.REGIMES:
            data = case(regime, R, C, bad)[0]
            got = {m for m in KR.MUTANTS if not KR.mutant_applies(m, data, plans)[0]}
            if regime in ("flat", "shifted"):
                assert got == want[(R, C)], (regime, R, C, got)
            else:
                assert want[(R, C)] <= got <= want[(R, C)] | {"padded_column_counted"}, (regime, R, C, got)


def test_plans_at_the_table_shapes():
    """What each shape of the table reaches, as the launchers' own arithmetic reports it."""
    assert plan(0, 1, 2)[:5] == [1, 1, 1, 1, 16]
    assert plan(0, 21, 64)[:5] == [1, 1, 1, 1, 32]
    assert plan(0, 21, 65)[:5] == [2, 2, 1, 2, 32]
    assert plan(0, 84, 121)[:5] == [2, 2, 1, 2, 96] and plan(1, 84, 121)[:4] == [1, 4, 1, 3]
    assert plan(0, 1000, 2081)[:5] == [32, 8, 7, 33, 1008] and plan(1, 1000, 2081)[:4] == [2, 33, 1, 32]
    assert plan(0, 2081, 2081)[:5] == [23, 7, 7, 33, 2096] and plan(1, 2081, 2081)[:4] == [2, 33, 2, 33]
    assert plan(0, 130, 4097)[:5] == [32, 8, 1, 65, 144] and plan(1, 130, 4097)[:4] == [4, 33, 1, 5]
    assert plan(2, 84, 121) == [0] * 8
