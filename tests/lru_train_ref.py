"""Float64 reference, element-wise error bounds, an fp32 emulation and mutants for the item GEMM + softmax cross-entropy of the
retriever's training step, in its three forms (csrc/lru_train_scores.hip, csrc/lru_train_ce.hip, and the generic GEMM launches
around tr_ce_kernel in csrc/lru_train.hip), reached alone through lr_lru_train_ce_parity.
Test infrastructure only: tests/test_lru_train_ref_host.py pins it on the CPU (the emulation inside every bound, every mutant
outside, on the data the GPU test uses), tests/test_gpu_lru_train_ce_bounds.py compares the HIP kernels with it.

Conventions (those of tests/lora_kernels_ref.py). eps = 2^-24, the relative error of one fp32 operation; ulp32(v) the fp32 step
at 1.01 |v|. The *reference* is float64 with nothing rounded; a *bound* is derived from the fp32 operations a kernel performs and
is never fitted to a kernel's output; the *emulation* performs the arithmetic in fp32 numpy with another summation order; a
*mutant* is the reference with one plausible kernel bug.

The operation. s_rj = x_r . e_j + b_j; a row is valid when 0 < label < C; n = number of valid rows; lse_r = log sum_j exp s_rj;
p_rj = exp(s_rj - lse_r); dl_rj = (p_rj - [j = label_r]) / n on valid rows, 0 elsewhere; loss sum = sum_r (lse_r - s_r,label);
dX = dl E, dE = dl^T x, dbias = column sums of dl.

One formula per output, chain lengths per form. The three forms perform the same operations per element and differ in how long
their chains of additions are (an item split of form 0 adds 64 ceil(nsb / ns2) terms one after the other, the unsplit generic
product of form 2 all C of them), so the bounds below are written once over four chain lengths -- T_s (additions behind one
row's sum of exponentials), T_m (rescalings of a running sum to a new maximum), T_x (additions behind one d x element), T_e
(behind one d E / d bias element) -- and chains(form, R, C, plan) derives those from the launch plan lr_lru_train_ce_plan
reports. One bound for all forms would have to carry form 2's T_x = C at every shape, eight times form 0's at C = 4097, and let
an error through that a split's lost partial sum makes; per-form chains keep each form's bound at its own arithmetic.

logit      sigma_rj = (64 + 3) eps (sum_k |x_rk e_jk| + |b_j|): 64 products summed with the bias in one MFMA chain (65 additions),
           and in form 0 x and the bias are first multiplied by log2 e (one rounding each) and the logit lives in the log2 domain,
           one more rounding of |s|: 64 + 2, plus that one.
sum of exp every term exp(s'_j - m') carries sigma_rj (the argument moved), 2 eps |s_j - m| (the subtraction; the product by log2 e
           inside __expf) and the instruction's 2^-22. A running sum is rescaled by exp(m_old - m_new) whenever the maximum
           grows: the arguments telescope to at most m - s_j (2 eps (m - s_j) more) and each of at most T_m rescalings adds
           2^-22 + eps. All terms are positive, so T_s additions are T_s eps relative.
           e_S = max_j sigma_rj + 4 eps sum_j p_j (m - s_j) + (T_m + 1) (2^-22 + eps) + T_s eps + C 2^-120 (flushed terms)
lse        D_lse = e_S + 2^-22 (|log S| + log n + 1) + 4 eps (|lse| + log n): the logarithm (form 0 takes a second one, log2 n,
           to fold 1 / n into the exponent), the additions m + log S (+ log2 n).
softmax    p' / n relative rho_rj = sigma_rj + D_lse + 2^-22 (|s_rj - lse_r| + log n + 2) + 4 eps (1 / n, its product, in form 2
           the product by 1 / sum). Where s - lse - log n < -86 the result leaves v_exp_f32's normal range and may be flushed
           to zero: rho gains 1 there (the bound gains p itself).
d x        sum_j p rho |e_jd| / n + T_x eps sum_j (p_rj + [j = label]) |e_jd| / n + 3 eps |e_label,d| / n: the softmax's own
           error, the chain (forms 1 and 2 subtract the one-hot inside the term, form 0 adds it as a term of its own: the
           sum of magnitudes covers both), the one-hot's roundings (1 / n, the product, the subtraction from p).
d E, d b   the same over rows with |x_rd| (1 for the bias) and T_e, the one-hot at every row that carries label j, plus ulp32
           of the result: the buffers hold a value already.
loss sum   per row D_lse + sigma_r,label + eps (|lse| + |s_label|) + eps |loss_r|, then (n + 2) eps sum_r |loss_r| for the sum
           (one atomic per row in forms 1 and 2, a four-row tree and one atomic per workgroup in form 0).

chains     form 0  T_s = 2 (4 sb + 2) + 8, T_m = 4 sb + 2 + 1 with sb = ceil(nsb / ns) super-blocks per split (four 4-item steps
                   each, two shuffle merges, one combine whose tree over <= 32 partials is 6 deep: the 8);
                   T_x = 64 ceil(nsb / ns2) + ns2 + 2 (the one-hot is in d x before the splits add);
                   T_e = 16 ceil(ceil(Rpad / 16 / nq) / 4) + 4 + nq + n_max + 2, n_max the most rows with one label (every
                   labelled row adds its one-hot with an atomic of its own).
           form 1  a lane sums 16 items of each 32-item tile of its chunk, then the lane halves, then the chunks:
                   T_s = 17 tiles + chunks + 4, T_m = tiles + chunks + 1; T_x = 32 tiles + chunks + 2; T_e = 32 row tiles +
                   row chunks + 2.
           form 2  256 threads stride the row, then a 6 + 3 step tree: T_s = ceil(C / 256) + 10, T_m = 0. The generic products
                   split K over S workgroups: ceil(K / S) + S <= K + 1 for any S, so T_x = C + 2 and T_e = R + 2 without
                   restating the launcher's choice of S.
"""
from __future__ import annotations

import functools

import numpy as np

from llamarec_amd.synth import hash_uniform, splitmix64

EPS = 2.0 ** -24
U22 = 2.0 ** -22
FLUSH = -86.0

MUTANTS = ("padded_column_counted", "last_tile_missing_from_dE", "partials_not_rescaled", "ragged_panel_rows_missing",
           "n_counts_bad_labels", "onehot_at_label_minus_one")

# (R, C, bad labels): tests/test_gpu_lru_train_ce_bounds.py runs every one for all forms and regimes
SHAPES = ((1, 2, False), (21, 64, False), (21, 65, False), (84, 121, False), (1000, 2081, False), (2081, 2081, True),
          (130, 4097, False))
REGIMES = ("flat", "peaked", "wide", "shifted")


def ulp32(v):
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)) * 1.01, 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite, or differs at all where the bound is zero (an element no term
    reaches: it must be the reference's exact value)."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - np.asarray(ref, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    if (err[bound == 0] != 0).any():
        return float("inf")
    return float((err / np.where(bound == 0, 1.0, bound)).max())


# ---- data --------------------------------------------------------------------------------------------------------------------
def ce_labels(R, C, seed, bad=False):
    """Uniform in 1..V; every fifth row (r % 5 == 4) has label 0; with bad, four rows carry 10**6 or -5."""
    V = C - 1
    lab = ((splitmix64(seed + 7, R) >> np.uint64(20)) % np.uint64(V)).astype(np.int64) + 1
    lab[np.arange(R) % 5 == 4] = 0
    if bad:
        for i, r in enumerate((3, R // 3, R // 2, R - 7)):
            lab[r] = 10 ** 6 if i % 2 == 0 else -5
    return lab


def ce_data(regime, R, C, seed, bad=False):
    """(x [R][64], E [C][64], bias [C]) float32, labels int64 [R]. Built from hash_uniform and rounded to fp32 once, on the
    host: the GPU gets these bits.
    flat: x unit scale (the final LayerNorm's output), table std 0.02, bias std 0.02: logits near 0, loss near ln C.
    peaked: flat, with x_r moved along e_label so that the label's logit gains 20: p - 1 cancels at the label.
    wide: table std 1.6: logits of standard deviation 13, spread over about +-40.
    shifted: flat with every bias at -60: a padded column's 0 is far above every real logit."""
    lab = ce_labels(R, C, seed, bad)
    x = hash_uniform(seed + 1, (R, 64), 1.0)
    E = hash_uniform(seed + 2, (C, 64), 1.6 if regime == "wide" else 0.02)
    bias = hash_uniform(seed + 3, (C,), 0.02)
    if regime == "shifted":
        bias = np.full(C, -60.0, np.float32)
    elif regime == "peaked":
        ok = (lab > 0) & (lab < C)
        el = E[np.where(ok, lab, 0)].astype(np.float64)
        x = (x + np.where(ok[:, None], 20.0 * el / (el * el).sum(1, keepdims=True), 0.0)).astype(np.float32)
    elif regime not in ("flat", "wide"):
        raise ValueError(regime)
    return x, E, bias, lab


# ---- reference and mutants -----------------------------------------------------------------------------------------------------
def _forward64(x, E, bias, labels):
    C = E.shape[0]
    valid = (labels > 0) & (labels < C)
    s = x @ E.T + bias
    m = s.max(1)
    ex = np.exp(s - m[:, None])
    S = ex.sum(1)
    return valid, s, m, ex, S


def ce_ref64(x, E, bias, labels, mutant=None, splits=2):
    """float64 x [R][64], E [C][64], bias [C], int labels [R] -> (loss sum, n, dX, dE, dbias). Invalid rows (label 0 or out of
    range) contribute nothing; n is the number of valid rows. mutant: one of MUTANTS (splits: item splits of
    partials_not_rescaled, over 64-item super-blocks as form 0 splits them)."""
    x, E, bias = (np.asarray(a, dtype=np.float64) for a in (x, E, bias))
    labels = np.asarray(labels, dtype=np.int64)
    R, C = x.shape[0], E.shape[0]
    valid, s, m, ex, S = _forward64(x, E, bias, labels)
    n = int(valid.sum())
    if mutant == "n_counts_bad_labels":
        n = int((labels != 0).sum())
    if mutant == "padded_column_counted":   # logit 0 on the items C .. up to the 64-item pitch
        pad = (-C) % 64
        m2 = np.maximum(m, 0.0)
        S = S * np.exp(m - m2) + pad * np.exp(-m2)
        ex = ex * np.exp(m - m2)[:, None]
        m = m2
    if mutant == "partials_not_rescaled":   # sum of the splits' sums, each still at its own maximum
        nsb = (C + 63) // 64
        S = np.zeros(R)
        for k in range(splits):
            a, b = 64 * (k * nsb // splits), min(C, 64 * ((k + 1) * nsb // splits))
            if a < b:
                S += np.exp(s[:, a:b] - s[:, a:b].max(1, keepdims=True)).sum(1)
    lse = m + np.log(S)
    p = ex / S[:, None]
    lab = np.where(valid, labels, 0)
    rows = np.arange(R)
    loss = float(((lse - s[rows, lab]) * valid).sum())
    w = valid / max(n, 1)
    soft = p * w[:, None]
    hot = np.zeros_like(p)
    hot[rows, lab - 1 if mutant == "onehot_at_label_minus_one" else lab] = w
    dl = soft - hot
    dX = dl @ E
    dl_e = dl
    if mutant == "last_tile_missing_from_dE":
        dl_e = dl.copy()
        t0 = 32 * ((C - 1) // 32)
        dl_e[:, t0:] = -hot[:, t0:]
    if mutant == "ragged_panel_rows_missing":
        dl_e = dl.copy()
        dl_e[R - R % 16:] = 0.0
    return loss, n, dX, dl_e.T @ x, dl_e.sum(0)


def mutant_applies(mutant, data, plans):
    """Whether `mutant` can differ from the reference on data = (x, E, bias, labels), and if not, why (by name, never
    silently). plans: {form: lr_lru_train_ce_plan's 8 values}."""
    x, E, bias, labels = data
    labels = np.asarray(labels)
    R, C = len(labels), E.shape[0]
    valid = (labels > 0) & (labels < C)
    if not valid.any():
        return False, "no labelled row"
    if mutant == "padded_column_counted":
        if C % 64 == 0:
            return False, "no padded column: C is a multiple of the 64-item pitch"
        _, _, m, _, S = _forward64(*(np.asarray(a, dtype=np.float64) for a in (x, E, bias)), labels)
        if ((-C) % 64 * np.exp(-(m + np.log(S)))[valid]).max() < U22:
            return False, ("every labelled row's lse is so far above 0 that the padded columns add under 2^-22 of its sum of "
                           "exponentials, less than the error of the one v_exp_f32 every bound must allow")
    if mutant == "partials_not_rescaled" and plans[0][0] == 1 and plans[1][0] == 1:
        return False, "one item split in form 0 and one item chunk in form 1: nothing to rescale"
    if mutant == "ragged_panel_rows_missing":
        if R % 16 == 0:
            return False, "R is a multiple of the 16-row panel"
        if not valid[R - R % 16:].any():
            return False, "no labelled row in the last panel"
    if mutant == "n_counts_bad_labels" and not ((labels < 0) | (labels >= C)).any():
        return False, "no out-of-range label in the data"
    return True, ""


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def chains(form, R, C, plan, labels):
    """(T_s, T_m, T_x, T_e) of a form at a shape (module docstring); plan = lr_lru_train_ce_plan(form, R, C)."""
    labels = np.asarray(labels)
    valid = (labels > 0) & (labels < C)
    n_max = int(np.bincount(labels[valid]).max()) if valid.any() else 0
    cdiv = lambda a, b: -(-a // b)
    if form == 0:
        ns, ns2, nq, nsb, rpad = (int(v) for v in plan[:5])
        sb = cdiv(nsb, ns)
        return (2 * (4 * sb + 2) + 8, 4 * sb + 3, 64 * cdiv(nsb, ns2) + ns2 + 2,
                16 * cdiv(cdiv(rpad // 16, nq), 4) + 4 + nq + n_max + 2)
    if form == 1:
        ic, it, rc, rt = (int(v) for v in plan[:4])
        return 17 * it + ic + 4, it + ic + 1, 32 * it + ic + 2, 32 * rt + rc + 2
    if form == 2:
        return cdiv(C, 256) + 10, 0, C + 2, R + 2
    raise ValueError(form)


def ce_bounds(x, E, bias, labels, T, base_dE=None, base_dbias=None):
    """float64 inputs, T = chains(...) -> dict of bounds: loss (scalar), dX [R][64], dE [C][64], dbias [C]. base_*: what the
    gradient buffers held before the call (the ulp32 term is taken at base + result)."""
    T_s, T_m, T_x, T_e = T
    x, E, bias = (np.asarray(a, dtype=np.float64) for a in (x, E, bias))
    labels = np.asarray(labels, dtype=np.int64)
    R, C = x.shape[0], E.shape[0]
    valid, s, m, ex, S = _forward64(x, E, bias, labels)
    n = max(int(valid.sum()), 1)
    ln_n = np.log(n)
    lse = m + np.log(S)
    p = ex / S[:, None]
    ax, aE = np.abs(x), np.abs(E)
    sigma = (64 + 3) * EPS * (ax @ aE.T + np.abs(bias))
    e_S = sigma.max(1) + 4 * EPS * (p * (m[:, None] - s)).sum(1) + (T_m + 1) * (U22 + EPS) + T_s * EPS + C * 2.0 ** -120
    D_lse = e_S + U22 * (np.abs(np.log(S)) + ln_n + 1) + 4 * EPS * (np.abs(lse) + ln_n)
    arg = s - lse[:, None]
    rho = sigma + D_lse[:, None] + U22 * (np.abs(arg) + ln_n + 2) + 4 * EPS
    rho = rho + (arg - ln_n < FLUSH)
    w = valid / n
    lab = np.where(valid, labels, 0)
    rows = np.arange(R)
    hot = np.zeros_like(p)
    hot[rows, lab] = w
    perr = p * rho * w[:, None]             # the softmax term's own error, per element of dl
    mag = p * w[:, None] + hot              # magnitudes of the terms a chain adds
    dX = perr @ aE + T_x * EPS * (mag @ aE) + 3 * EPS * (hot @ aE)
    dE = perr.T @ ax + T_e * EPS * (mag.T @ ax) + 3 * EPS * (hot.T @ ax)
    db = perr.sum(0) + T_e * EPS * mag.sum(0) + 3 * EPS * hot.sum(0)
    _, _, _, rE, rb = ce_ref64(x, E, bias, labels)
    dE = dE + ulp32(rE + (0.0 if base_dE is None else np.asarray(base_dE, dtype=np.float64)))
    db = db + ulp32(rb + (0.0 if base_dbias is None else np.asarray(base_dbias, dtype=np.float64)))
    s_lab = s[rows, lab]
    loss_r = (lse - s_lab) * valid
    per_row = (D_lse + sigma[rows, lab] + EPS * (np.abs(lse) + np.abs(s_lab)) + EPS * np.abs(loss_r)) * valid
    loss = float(per_row.sum() + (n + 2) * EPS * np.abs(loss_r).sum())
    return {"loss": loss, "dX": dX, "dE": dE, "dbias": db}


# ---- fp32 emulation --------------------------------------------------------------------------------------------------------------
def ce_emul32(x, E, bias, labels, item_splits=1, row_parts=1, order="fwd"):
    """The same arithmetic in fp32 numpy: logits as an fp32 matrix product over k forwards or backwards (`order` "fwd" / "rev",
    which also reverses the order the splits, parts and rows are added in) plus the bias, (max, sum) partials per item split
    rescaled to the common maximum, lse = m + log S, p = exp(s - lse), gradients as per-split / per-part fp32 products added in
    turn. -> (loss sum, n, dX, dE, dbias) float32."""
    f = np.float32
    x, E, bias = (np.asarray(a, dtype=f) for a in (x, E, bias))
    labels = np.asarray(labels, dtype=np.int64)
    R, C = x.shape[0], E.shape[0]
    valid = (labels > 0) & (labels < C)
    n = int(valid.sum())
    if order == "fwd":
        s = (x @ E.T + bias).astype(f)
    else:
        s = (np.ascontiguousarray(x[:, ::-1]) @ np.ascontiguousarray(E[:, ::-1]).T + bias).astype(f)
    edges = [C * k // item_splits for k in range(item_splits + 1)]
    parts = [(a, b) for a, b in zip(edges[:-1], edges[1:]) if a < b]
    mk = [s[:, a:b].max(1) for a, b in parts]
    sk = [np.exp(s[:, a:b] - mk_[:, None]).astype(f).sum(1, dtype=f) for (a, b), mk_ in zip(parts, mk)]
    m = functools.reduce(np.maximum, mk)
    S = np.zeros(R, f)
    for mk_, sk_ in (zip(mk, sk) if order == "fwd" else zip(mk[::-1], sk[::-1])):
        S = S + sk_ * np.exp(mk_ - m).astype(f)
    lse = (m + np.log(S).astype(f)).astype(f)
    lab = np.where(valid, labels, 0)
    rows = np.arange(R)
    loss = f(0)
    for r in (rows if order == "fwd" else rows[::-1]):
        if valid[r]:
            loss = f(loss + f(lse[r] - s[r, lab[r]]))
    inv_n = f(1) / f(max(n, 1))
    p = np.exp(s - lse[:, None]).astype(f)
    p[rows, lab] -= f(1)
    dl = (p * inv_n * valid[:, None].astype(f)).astype(f)
    dX = np.zeros((R, 64), f)
    for a, b in (parts if order == "fwd" else parts[::-1]):
        dX = dX + (dl[:, a:b] @ E[a:b]).astype(f)
    redges = [R * k // row_parts for k in range(row_parts + 1)]
    rparts = [(a, b) for a, b in zip(redges[:-1], redges[1:]) if a < b]
    dE, db = np.zeros((C, 64), f), np.zeros(C, f)
    for a, b in (rparts if order == "fwd" else rparts[::-1]):
        dE = dE + (dl[a:b].T @ x[a:b]).astype(f)
        db = db + dl[a:b].sum(0, dtype=f)
    return float(loss), n, dX, dE, db
