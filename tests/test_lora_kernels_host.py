"""CPU: the stand-alone entry points of the LoRA step's small kernels (header, prototypes, every host-side refusal through the
library loaded without a GPU) and tests/lora_kernels_ref.py itself: on the data the GPU tests use, every fp32 emulation sits
inside its derived bound and every mutant outside; the dropout restatement equals the oracle's mask; the float64 references of
the three backward formulas equal torch's float64 autograd of the plain forward."""
import os
import re

import numpy as np
import torch

from tests import lora_kernels_ref as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_EINVAL, LR_EUNSUPPORTED, LR_EWORKSPACE = -1, -2, -4
NEW_SYMBOLS = ("lr_lora_skinny_bf16", "lr_lora_tn_det_floats", "lr_lora_tn_f32", "lr_lora_expand_bf16", "lr_swiglu_fwd_bf16",
               "lr_swiglu_bwd_bf16", "lr_rmsnorm_bwd_bf16", "lr_ce_bf16", "lr_rowdot_bf16", "lr_lora_adamw_f32",
               "lr_lora_rope_fwd_bf16", "lr_rope_bwd_bf16", "lr_swiglu_lora_fwd_bf16", "lr_lora_prep_bf16", "lr_lora_prep_module_bf16")


def test_header_prototypes_and_library_agree():
    from llamarec_amd import _lib

    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    section = header[header.index("The LoRA step's small kernels alone (exposed for parity tests)"):]
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, section, flags=re.S)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert n_args == len(_lib.PROTOTYPES[name][1]), (name, n_args)
        assert hasattr(l, name)
        if name != "lr_lora_tn_det_floats":
            assert "void* hip_stream" in decl.group(1).split(",")[-1], name   # flat C arguments, the stream last


# an aligned and a misaligned fake device address: the refusals below come before anything dereferences or launches
A, B, ODD = 0x10000, 0x20000, 0x10004


def _refused(rc, code, *words):
    from llamarec_amd import _lib

    msg = _lib.lib().lr_last_error()
    assert rc == code, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_every_wrapper_refuses_what_its_kernel_assumes():
    from llamarec_amd import _lib

    l = _lib.lib()
    # rank-r product
    _refused(l.lr_lora_skinny_bf16(None, 64, 4, 64, B, 1, A, 16, 0, 1.0, 0, 0.0, None), LR_EINVAL, "null")
    _refused(l.lr_lora_skinny_bf16(A, 64, -1, 64, B, 1, A, 16, 0, 1.0, 0, 0.0, None), LR_EINVAL, "n -1")
    _refused(l.lr_lora_skinny_bf16(A, 64, 4, 64, B, 3, A, 64, 0, 1.0, 0, 0.0, None), LR_EINVAL, "3 tiles")
    _refused(l.lr_lora_skinny_bf16(A, 64, 4, 64, B, 2, A, 40, 16, 1.0, 0, 0.0, None), LR_EINVAL, "column 16 of 40")
    _refused(l.lr_lora_skinny_bf16(A, 56, 4, 64, B, 1, A, 16, 0, 1.0, 0, 0.0, None), LR_EINVAL, "ldx 56")
    _refused(l.lr_lora_skinny_bf16(A, 64, 4, 64, B, 1, A, 16, 0, 1.0, 0, 1.0, None), LR_EINVAL, "dropout 1")
    _refused(l.lr_lora_skinny_bf16(A, 64, 4, 64, B, 1, A, 16, 0, 1.0, 0, -0.1, None), LR_EINVAL, "dropout")
    _refused(l.lr_lora_skinny_bf16(A, 96, 4, 96, B, 1, A, 16, 0, 1.0, 0, 0.0, None), LR_EUNSUPPORTED, "multiple of 64")
    _refused(l.lr_lora_skinny_bf16(A, 68, 4, 64, B, 1, A, 16, 0, 1.0, 0, 0.0, None), LR_EUNSUPPORTED, "ldx 68")
    _refused(l.lr_lora_skinny_bf16(ODD, 64, 4, 64, B, 1, A, 16, 0, 1.0, 0, 0.0, None), LR_EUNSUPPORTED, "aligned")

    # token reduction
    def tn(nj=1, t=A, ldt=32, tcol=0, x=B, ldx=64, n=4, cols=64, o0=A, o1=None, r=8, layout=0, hd=0, p=0.0, part=None, pf=0):
        return l.lr_lora_tn_f32(nj, t, ldt, tcol, x, ldx, n, cols, 1.0, o0, o1, r, layout, hd, 0, p, part, pf, None)

    _refused(tn(t=None), LR_EINVAL, "null")
    _refused(tn(nj=3), LR_EINVAL, "3 tiles")
    _refused(tn(n=-1), LR_EINVAL, "n -1")
    _refused(tn(r=0), LR_EINVAL, "r 0")
    _refused(tn(r=17), LR_EINVAL, "r 17")
    _refused(tn(layout=4), LR_EINVAL, "layout 4")
    _refused(tn(nj=2, o1=B, tcol=8, ldt=32), LR_EINVAL, "column 8 of 32")
    _refused(tn(cols=128, ldx=64), LR_EINVAL, "cols 128 <= ldx 64")
    _refused(tn(p=1.5), LR_EINVAL, "dropout")
    _refused(tn(o0=None), LR_EINVAL, "null output")
    _refused(tn(nj=2, ldt=32, o1=None), LR_EINVAL, "null output")
    _refused(tn(nj=2, layout=3, o0=None, o1=None), LR_EINVAL, "null output")
    _refused(tn(nj=1, layout=3), LR_EINVAL, "null output")
    _refused(tn(cols=96, ldx=96), LR_EUNSUPPORTED, "multiple of 64")
    _refused(tn(layout=2, hd=0), LR_EUNSUPPORTED, "head_dim 0")
    _refused(tn(layout=2, hd=48), LR_EUNSUPPORTED, "head_dim 48")
    _refused(tn(o0=0x10002), LR_EINVAL, "misaligned")
    need = l.lr_lora_tn_det_floats(1, 4, 64, 8, 0)
    assert need == 8 * 64
    _refused(tn(part=A, pf=need - 1), LR_EWORKSPACE, "partial tiles")
    _refused(tn(part=ODD, pf=need), LR_EUNSUPPORTED, "16-byte aligned")
    _refused(tn(o0=ODD, part=A, pf=need), LR_EUNSUPPORTED, "16-byte aligned")
    assert tn(n=0) == 0    # nothing to do, nothing launched

    # expand-add
    def ex(y=A, ldy=64, n=4, cols=64, t=B, ldt=16, tcol=0, w=B, r=8, p=0.0):
        return l.lr_lora_expand_bf16(y, ldy, n, cols, t, ldt, tcol, w, r, 1.0, 0, p, None)

    _refused(ex(w=None), LR_EINVAL, "null")
    _refused(ex(n=-2), LR_EINVAL, "n -2")
    _refused(ex(cols=72), LR_EINVAL, "cols 72 <= ldy 64")
    _refused(ex(r=0), LR_EINVAL, "r 0")
    _refused(ex(tcol=8), LR_EINVAL, "column 8 of 16")
    _refused(ex(p=1.0), LR_EINVAL, "dropout")
    _refused(ex(cols=12), LR_EUNSUPPORTED, "cols 12")
    _refused(ex(ldy=68), LR_EUNSUPPORTED, "ldy 68")
    _refused(ex(y=ODD), LR_EUNSUPPORTED, "aligned")
    _refused(ex(w=ODD), LR_EUNSUPPORTED, "aligned")

    # SwiGLU
    for fn, name in ((l.lr_swiglu_fwd_bf16, "lr_swiglu_fwd_bf16"), (l.lr_swiglu_bwd_bf16, "lr_swiglu_bwd_bf16")):
        _refused(fn(None, B, 4, 16, None), LR_EINVAL, name)
        _refused(fn(A, B, -1, 16, None), LR_EINVAL, "n -1")
        _refused(fn(A, B, 4, 0, None), LR_EINVAL, "f 0")
        _refused(fn(A, B, 4, 24, None), LR_EUNSUPPORTED, "intermediate size 24")
        _refused(fn(A, ODD, 4, 16, None), LR_EUNSUPPORTED, name)

    # RMSNorm backward
    def nb(dy=A, x=B, w=A, res=None, out=B, rows=4, d=64, eps=1e-5, dt=None, ldt=32, a_cat=None, r=8, p=0.0):
        return l.lr_rmsnorm_bwd_bf16(dy, x, w, res, out, rows, d, eps, None, dt, ldt, a_cat, r, 0, p, None)

    _refused(nb(out=None), LR_EINVAL, "null")
    _refused(nb(rows=-1), LR_EINVAL, "rows -1")
    _refused(nb(eps=-1.0), LR_EINVAL, "eps")
    _refused(nb(p=1.0), LR_EINVAL, "dropout")
    _refused(nb(dt=A), LR_EINVAL, "a_cat")
    _refused(nb(dt=A, a_cat=B, r=17), LR_EINVAL, "r 17")
    _refused(nb(dt=A, a_cat=B, ldt=16), LR_EINVAL, "ldt 16")
    _refused(nb(d=12), LR_EUNSUPPORTED, "hidden_size 12")
    _refused(nb(d=8200), LR_EUNSUPPORTED, "hidden_size 8200")
    _refused(nb(res=ODD), LR_EUNSUPPORTED, "aligned")
    _refused(nb(dt=A, a_cat=ODD), LR_EUNSUPPORTED, "aligned")

    # loss head, rowdot, AdamW
    _refused(l.lr_ce_bf16(A, 4, 320, None, 1.0, B, A, 0, None), LR_EINVAL, "lr_ce_bf16")
    _refused(l.lr_ce_bf16(A, -1, 320, B, 1.0, B, A, 0, None), LR_EINVAL, "m -1")
    _refused(l.lr_ce_bf16(A, 4, 0, B, 1.0, B, A, 0, None), LR_EINVAL, "vocab 0")
    _refused(l.lr_rowdot_bf16(A, None, 4, 2, 64, B, None), LR_EINVAL, "lr_rowdot_bf16")
    _refused(l.lr_rowdot_bf16(A, B, -4, 2, 64, B, None), LR_EINVAL, "n -4")
    _refused(l.lr_rowdot_bf16(A, B, 2 ** 30, 4, 64, B, None), LR_EINVAL, "heads")
    _refused(l.lr_rowdot_bf16(A, B, 4, 2, 12, B, None), LR_EUNSUPPORTED, "head_dim 12")
    _refused(l.lr_rowdot_bf16(ODD, B, 4, 2, 64, B, None), LR_EUNSUPPORTED, "head_dim 64")

    def aw(p=A, g=B, n=8, ctr=A, b1=0.9, b2=0.999, eps=1e-8, det=0):
        return l.lr_lora_adamw_f32(p, g, A, B, n, A, ctr, 1e-3, 1.0, b1, b2, eps, 0.0, None, det, None)

    _refused(aw(ctr=None), LR_EINVAL, "null")
    _refused(aw(b1=1.0), LR_EINVAL, "betas")
    _refused(aw(b2=-0.5), LR_EINVAL, "betas")
    _refused(aw(eps=-1.0), LR_EINVAL, "eps")
    _refused(aw(g=ODD, det=1), LR_EUNSUPPORTED, "16-byte aligned")
    assert aw(n=0) == 0

    # forward sweep
    def rf(qkv=A, n=4, qw=512, qc=256, kc=128, hd=64, t=B, bq=A, bv=B, r=8, pos=A, cs=B, tk=None, ldtk=16, tkcol=0, bk=None,
           qn=None, kn=None, eps=1e-6, xs=None):
        return l.lr_lora_rope_fwd_bf16(qkv, n, qw, qc, kc, hd, t, bq, bv, r, 4.0, pos, cs, tk, ldtk, tkcol, bk, qn, kn, eps, xs, None)

    _refused(rf(bv=None), LR_EINVAL, "null")
    _refused(rf(n=-1), LR_EINVAL, "n -1")
    _refused(rf(r=17), LR_EINVAL, "r 17")
    _refused(rf(qc=512, kc=128), LR_EINVAL, "q 512 + k 128 columns of 512")
    _refused(rf(bk=A), LR_EINVAL, "k adapter")
    _refused(rf(bk=A, tk=B, tkcol=8), LR_EINVAL, "column 8 + 16 <= ldtk 16")
    _refused(rf(kn=A), LR_EINVAL, "without a q norm")
    _refused(rf(xs=A), LR_EINVAL, "without a q norm")
    _refused(rf(qn=A, kn=B, xs=A, eps=-1.0), LR_EINVAL, "eps")
    _refused(rf(qn=A, xs=A), LR_EINVAL, "null k norm or save buffer")
    _refused(rf(qn=A, kn=B), LR_EINVAL, "null k norm or save buffer")
    _refused(rf(hd=12, qc=240, kc=120, qw=480), LR_EUNSUPPORTED, "head_dim 12")
    _refused(rf(hd=64, qc=200), LR_EUNSUPPORTED, "divide")
    _refused(rf(qw=516), LR_EUNSUPPORTED, "row stride 516")
    _refused(rf(hd=96, qc=192, kc=96, qw=384, qn=A, kn=B, xs=A), LR_EUNSUPPORTED, "head_dim 96")
    _refused(rf(qkv=ODD), LR_EUNSUPPORTED, "aligned")
    _refused(rf(qn=ODD, kn=B, xs=A), LR_EUNSUPPORTED, "aligned")
    assert rf(n=0) == 0

    # rotation backward
    _refused(l.lr_rope_bwd_bf16(A, 4, 512, 384, 64, None, B, None), LR_EINVAL, "null")
    _refused(l.lr_rope_bwd_bf16(A, -4, 512, 384, 64, A, B, None), LR_EINVAL, "n -4")
    _refused(l.lr_rope_bwd_bf16(A, 4, 256, 384, 64, A, B, None), LR_EINVAL, "384 rotated columns of 256")
    _refused(l.lr_rope_bwd_bf16(ODD, 4, 512, 384, 64, A, B, None), LR_EUNSUPPORTED, "aligned")
    _refused(l.lr_rope_bwd_bf16(A, 4, 512, 384, 12, A, B, None), LR_EUNSUPPORTED, "head_dim 12")   # the launcher's own checks
    _refused(l.lr_rope_bwd_bf16(A, 4, 512, 360, 64, A, B, None), LR_EUNSUPPORTED, "360 rotated columns")
    _refused(l.lr_rope_bwd_bf16(A, 4, 388, 384, 64, A, B, None), LR_EUNSUPPORTED, "of 388")
    assert l.lr_rope_bwd_bf16(A, 0, 512, 384, 64, A, B, None) == 0 and l.lr_rope_bwd_bf16(A, 4, 512, 0, 64, A, B, None) == 0

    # SwiGLU with adapters
    def sl(gu=A, h=B, n=4, f=16, t=A, ldt=32, tcol=0, w=B, r=8):
        return l.lr_swiglu_lora_fwd_bf16(gu, h, n, f, t, ldt, tcol, w, r, 4.0, None)

    _refused(sl(t=None), LR_EINVAL, "null")
    _refused(sl(n=-1), LR_EINVAL, "n -1")
    _refused(sl(r=0), LR_EINVAL, "r 0")
    _refused(sl(tcol=16), LR_EINVAL, "column 16 + 32 <= ldt 32")
    _refused(sl(f=40), LR_EUNSUPPORTED, "intermediate size 40")
    _refused(sl(w=ODD), LR_EUNSUPPORTED, "aligned")
    assert sl(n=0) == 0

    # working copies
    def pl(aq=A, r=8, d=64, qc=128, vc=64, hd=64, bvt=B):
        return l.lr_lora_prep_bf16(aq, B, A, B, r, d, qc, vc, hd, A, B, bvt, None)

    _refused(pl(aq=None), LR_EINVAL, "null")
    _refused(pl(bvt=None), LR_EINVAL, "null")
    _refused(pl(r=0), LR_EINVAL, "r 0")
    _refused(pl(d=0), LR_EINVAL, "hidden 0")
    _refused(pl(hd=63), LR_EINVAL, "head_dim 63")
    _refused(pl(qc=100), LR_EINVAL, "q 100")
    _refused(pl(d=2 ** 27), LR_EINVAL, "hidden")

    def pm(a=A, r=8, i=64, o=128, perm=0, hd=64, ldb=256, bt=B):
        return l.lr_lora_prep_module_bf16(a, B, r, i, o, perm, hd, A, bt, ldb, None)

    _refused(pm(bt=None), LR_EINVAL, "null")
    _refused(pm(r=17), LR_EINVAL, "r 17")
    _refused(pm(perm=4), LR_EINVAL, "perm 4")
    _refused(pm(ldb=127), LR_EINVAL, "ldb 127")
    _refused(pm(perm=2, ldb=255), LR_EINVAL, "ldb 255")
    _refused(pm(perm=1, hd=96), LR_EUNSUPPORTED, "head_dim 96")
    _refused(pm(perm=3, o=40, ldb=80), LR_EUNSUPPORTED, "out 40")


def test_det_floats_serve_every_smaller_batch():
    """The partial-tile count is not monotonic in n (511 tokens: 16 chunks of 32; 512: 4 of 128); what is asked for n must serve
    every smaller n."""
    from llamarec_amd import _lib

    l = _lib.lib()
    for nj, cols, r, layout in ((2, 320, 8, 0), (1, 64, 13, 1), (2, 192, 8, 3)):
        E = nj * r * cols // (2 if layout == 3 else 1)
        for n in K.TN_NS:
            have = l.lr_lora_tn_det_floats(nj, n, cols, r, layout)
            assert have % E == 0
            for k in K.TN_NS + (4095, 4096):
                if k <= n:
                    assert -(-k // K.tn_chunk(k)) * E <= have, (n, k)
    assert l.lr_lora_tn_det_floats(1, 0, 64, 8, 0) == 0 and l.lr_lora_tn_det_floats(3, 4, 64, 8, 0) == 0


def test_keep_restates_the_oracle_mask():
    from oracle import llama_train_oracle as O

    for seed, pas, layer, p in ((0, 0, 0, 0.05), (1234, 7, 3, 0.3), (2 ** 40 + 5, 1000, 31, 0.5)):
        stream = O.drop_stream(seed, pas, layer)
        mine = K.keep(stream, 37, 129, p)
        # the kernels take the threshold from the fp32 value of p: hand the oracle that value
        want = O.drop_mask(seed, pas, layer, 37, 129, float(np.float32(p))) > 0
        assert np.array_equal(mine, want)
        assert abs(mine.mean() - (1 - p)) < 0.03
    assert K.keep(5, 3, 9, 0.0).all()
    assert np.array_equal(K.keep(9, 5, 8, 0.3, row0=2)[:3], K.keep(9, 5, 8, 0.3)[2:])


def test_every_rotated_argument_value_reaches_the_cases_that_use_it():
    """The case lists rotate the secondary arguments instead of crossing them. Per operand kind: every listed value occurs, with
    every value of every other rotated argument and with every value of the shape arguments. A selector that follows the
    kind, or a value that lands only on cases that ignore it, fails here."""
    for kind in ("random", "exact"):
        sk = [c for c in K.skinny_cases() if c["kind"] == kind]
        assert {(c["n"], c["K"]) for c in sk} == {(n, k) for n in K.SKINNY_NS for k in K.SKINNY_KS}
        assert K.covered(sk, K.SKINNY_ROTATED, ("n", "K")) == []
        assert {c["p"] for c in sk} == {0.0, 0.3 if kind == "random" else 0.5}
        tn = [c for c in K.tn_cases() if c["kind"] == kind]
        assert {(c["n"], c["config"]) for c in tn} == {(n, k) for n in K.TN_NS for k in K.TN_CONFIGS}
        assert K.covered(tn, K.TN_ROTATED, ("n", "config")) == []
        assert {c["scale"] for c in tn} == set(K.TN_SCALES[kind])
        ex = [c for c in K.expand_cases() if c["kind"] == kind]
        assert {(c["n"], c["cols"]) for c in ex} == {(n, k) for n in K.EXPAND_NS for k in K.EXPAND_COLS}
        assert K.covered(ex, K.EXPAND_ROTATED, ("n", "cols")) == []
        assert {c["s"] for c in ex} == set(K.EXPAND_SCALES[kind]) and {c["p"] for c in ex} == {0.0, 0.3}
    # both kinds run the same arguments but for the values only one of them can take
    for cases in (K.skinny_cases, K.tn_cases, K.expand_cases):
        cs = list(cases())
        for rnd, exact in zip(cs[0::2], cs[1::2]):
            assert (rnd["kind"], exact["kind"]) == ("random", "exact")
            assert all(rnd[k] == exact[k] for k in rnd if k not in ("kind", "seed", "p", "scale", "s")), (rnd, exact)
    assert 1.4285714 in K.EXPAND_SCALES["random"]       # 1 / (1 - 0.3): not a power of two, so the chain's outer rounding counts
    norm = list(K.rmsnorm_cases())
    assert {(c["d"], c["rows"], c["lora"], c["res"], c["out_rows"]) for c in norm} >= {
        (d, rows, True, res, not res) for d in K.NORM_DS for rows in K.NORM_ROWS for res in (False, True)}
    assert K.covered([c for c in norm if c["lora"]], K.NORM_ROTATED, ("d", "rows", "res", "out_rows")) == []
    for d in K.NORM_DS:      # one width sees every (r, ldt, p)
        assert len({(c["r"], c["ldt"], c["p"]) for c in norm if c["lora"] and c["d"] == d}) == 12
    assert K.covered(list(K.rope_fwd_cases()), K.ROPE_ROTATED, ("inst", "hd", "n")) == []
    assert K.covered(list(K.adamw_cases()), dict(wd=(0.0, 0.01)), ("n", "step", "clip")) == []
    # the checker itself: a selector collinear with another argument, and a value that never occurs
    toy = [dict(a=i % 2, b=i % 2, n=i) for i in range(4)]
    assert ("a", 0, "b", 1) in K.covered(toy, dict(a=(0, 1), b=(0, 1))) and ("a", 2) in K.covered(toy, dict(a=(0, 1, 2)))


def _check(kernel, label, emul, ref, bound, worst):
    r = K.ratio(emul, ref, bound)
    worst[kernel] = max(worst.get(kernel, 0.0), r)
    assert r <= 1.0, (kernel, label, r)


def _mutant_outside(kernel, mutant, emul, mref, bound, label):
    r = K.ratio(emul, mref, bound)
    assert r > 1.0, (kernel, mutant, label, r)


def test_skinny_emulation_inside_and_mutants_outside():
    worst = {}
    for c in K.skinny_cases():
        x, w = K.skinny_data(c)
        ref, bound = K.skinny_ref64(x, w, c["scale"], K.STREAM, c["p"])
        em = K.skinny_emul32(x, w, c["scale"], K.STREAM, c["p"])
        _check("skinny", c, em, ref, bound, worst)
        if c["kind"] == "exact":
            assert np.array_equal(em.astype(np.float64), ref), c
        elif c["n"] == 67:
            for m in K.MUTANTS["skinny"]:
                _mutant_outside("skinny", m, em, K.skinny_ref64(x, w, c["scale"], K.STREAM, c["p"], mutant=m)[0], bound, c)
    print("skinny emulation: max err/bound %.3f" % worst["skinny"])


def _tn_mutant_applies(m, c):
    layout = K.TN_CONFIGS[c["config"]][0]
    n, chunk = c["n"], K.tn_chunk(c["n"])
    if m in ("last_partial_step_dropped", "tail_rows_not_zeroed"):
        return n % 32 != 0 and (m == "tail_rows_not_zeroed" or (n % chunk) % 32 != 0)
    return {"no_deinterleave": layout == 2, "gate_up_swapped": layout == 3, "assign_not_add": True}[m]


def test_token_reduction_emulation_inside_and_mutants_outside():
    worst, seen = {}, set()
    for c in K.tn_cases():
        layout, nj, cols, r, hd, have = K.TN_CONFIGS[c["config"]]
        t, x, init = K.tn_data(c)
        refs, bounds = K.tn_ref64(t, x, c["scale"], r, layout, hd, K.STREAM, c["p"], init)
        ems = K.tn_emul32(t, x, c["scale"], r, layout, hd, K.STREAM, c["p"], init)
        for a in range(2):
            assert (refs[a] is None) == (not have[a]) == (ems[a] is None)
            if refs[a] is None:
                continue
            _check("tn", c, ems[a], refs[a], bounds[a], worst)
            if c["kind"] == "exact":
                assert np.array_equal(ems[a].astype(np.float64), refs[a]), c
        if c["kind"] == "random" and c["n"] in (33, 100, 600):
            for m in K.MUTANTS["tn"]:
                if not _tn_mutant_applies(m, c):
                    continue
                mrefs, _ = K.tn_ref64(t, x, c["scale"], r, layout, hd, K.STREAM, c["p"], init, mutant=m)
                a = 0 if have[0] else 1
                _mutant_outside("tn", m, ems[a], mrefs[a], bounds[a], c)
                seen.add(m)
    assert seen == set(K.MUTANTS["tn"])
    print("token reduction emulation: max err/bound %.3f" % worst["tn"])


def test_expand_emulation_inside_and_mutants_outside():
    worst, seen = {}, set()
    for c in K.expand_cases():
        y, t, w = K.expand_data(c)
        ref, bound = K.expand_ref64(y, t, w, c["r"], c["s"], K.STREAM, c["p"])
        em = K.expand_emul32(y, t, w, c["r"], c["s"], K.STREAM, c["p"])
        _check("expand", c, em, ref, bound, worst)
        if c["kind"] == "exact":
            assert np.array_equal(em.astype(np.float64), ref), c
        elif c["n"] == 9 and c["cols"] >= 64:
            for m in K.MUTANTS["expand"]:
                if (m == "mask_of_next_row" and c["p"] == 0.0) or (m == "product_not_rounded" and (c["si"] == 0 or c["cols"] < 2048)):
                    continue
                _mutant_outside("expand", m, em, K.expand_ref64(y, t, w, c["r"], c["s"], K.STREAM, c["p"], mutant=m)[0], bound, c)
                seen.add(m)
    assert seen == set(K.MUTANTS["expand"])
    print("expand emulation: max err/bound %.3f" % worst["expand"])


def test_swiglu_backward_emulation_autograd_and_mutants():
    worst = {}
    for n in K.SWIGLU_NS:
        for f in K.SWIGLU_FS:
            g, u, dy = K.swiglu_data(n, f, seed=n + f)
            dg, du, bg, bu = K.swiglu_bwd_ref64(g, u, dy)
            eg, eu = K.swiglu_bwd_emul32(g, u, dy)
            _check("swiglu_bwd", (n, f, "dg"), eg, dg, bg, worst)
            _check("swiglu_bwd", (n, f, "du"), eu, du, bu, worst)
            gt = torch.from_numpy(g.astype(np.float64)).requires_grad_(True)
            ut = torch.from_numpy(u.astype(np.float64)).requires_grad_(True)
            (torch.nn.functional.silu(gt) * ut * torch.from_numpy(dy.astype(np.float64))).sum().backward()
            assert K.ratio(gt.grad.numpy(), dg, bg) <= 1.0 and K.ratio(ut.grad.numpy(), du, bu) <= 1.0
            if f >= 48:
                for m in K.MUTANTS["swiglu_bwd"]:
                    mg, mu, _, _ = K.swiglu_bwd_ref64(g, u, dy, mutant=m)
                    assert max(K.ratio(eg, mg, bg), K.ratio(eu, mu, bu)) > 1.0, (m, n, f)
    print("swiglu backward emulation: max err/bound %.3f" % worst["swiglu_bwd"])


def _norm_mutant_applies(m, c):
    return {"coef_missing": True, "mean_over_chunks": c["d"] % 2048 != 0, "res_before_rounding": c["res"] and c["rows"] >= 4,
            "mask_of_next_row": c["lora"] and c["p"] > 0}[m]


def test_rmsnorm_backward_emulation_autograd_and_mutants():
    worst, seen = {}, set()
    for c in K.rmsnorm_cases():
        dy, x, w, res, lora, _ = K.rmsnorm_data(c)
        ref, bound = K.rmsnorm_bwd_ref64(dy, x, w, 1e-5, res, lora)
        em = K.rmsnorm_bwd_emul32(dy, x, w, 1e-5, res, lora)
        _check("rmsnorm_bwd", c, em, ref, bound, worst)
        if not c["lora"] and not c["res"]:
            xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
            yt = torch.from_numpy(w.astype(np.float64)) * xt * torch.rsqrt((xt * xt).mean(-1, keepdim=True) + 1e-5)
            (yt * torch.from_numpy(dy.astype(np.float64))).sum().backward()
            assert K.ratio(xt.grad.numpy(), ref, bound) <= 1.0, c
        if c["d"] >= 64:
            for m in K.MUTANTS["rmsnorm_bwd"]:
                if not _norm_mutant_applies(m, c):
                    continue
                _mutant_outside("rmsnorm_bwd", m, em, K.rmsnorm_bwd_ref64(dy, x, w, 1e-5, res, lora, mutant=m)[0], bound, c)
                seen.add(m)
    assert seen == set(K.MUTANTS["rmsnorm_bwd"])
    print("rmsnorm backward emulation: max err/bound %.3f" % worst["rmsnorm_bwd"])


def test_cross_entropy_emulation_autograd_and_mutants():
    worst, seen = {}, set()
    for c in K.ce_cases():
        x, tg = K.ce_data(c["regime"], c["m"], c["V"], c["seed"])
        R = K.ce_ref64(x, tg, K.CE_GSCALE)
        grad, out = K.ce_emul32(x, tg, K.CE_GSCALE)
        _check("ce", (c, "grad"), grad, R["grad"], R["grad_bound"], worst)
        _check("ce", (c, "out"), out, R["out"], R["out_bound"], worst)
        live = (tg >= 0) & (tg < c["V"])
        if c["V"] <= 320 and live.any():
            xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
            loss = torch.nn.functional.cross_entropy(xt[live], torch.from_numpy(tg[live].astype(np.int64)), reduction="sum")
            (loss * float(np.float32(K.CE_GSCALE))).backward()
            assert K.ratio(xt.grad.numpy(), R["grad"], R["grad_bound"]) <= 1.0, c
            total = float(loss.detach())
            assert abs(total / c["m"] - R["out"][0]) <= R["out_bound"][0] + 1e-12 * abs(total)
        if c["m"] == 40 and c["regime"] in ("flat", "spike"):
            for m in K.MUTANTS["ce"]:
                M = K.ce_ref64(x, tg, K.CE_GSCALE, mutant=m)
                assert max(K.ratio(grad, M["grad"], R["grad_bound"]), K.ratio(out, M["out"], R["out_bound"])) > 1.0, (m, c)
                seen.add(m)
    assert seen == set(K.MUTANTS["ce"])
    print("cross-entropy emulation: max err/bound %.3f" % worst["ce"])


def test_rowdot_emulation_inside_and_mutant_outside():
    worst = {}
    for c in K.rowdot_cases():
        o, d_o = K.rowdot_data(c)
        ref, bound = K.rowdot_ref64(o, d_o)
        em = K.rowdot_emul32(o, d_o)
        _check("rowdot", c, em, ref, bound, worst)
        if c["kind"] == "exact":
            assert np.array_equal(em.astype(np.float64), ref)
        elif c["hd"] == 256:
            _mutant_outside("rowdot", "second_step_missing", em, K.rowdot_ref64(o, d_o, mutant="second_step_missing")[0], bound, c)
    print("rowdot emulation: max err/bound %.3f" % worst["rowdot"])


def test_adamw_emulation_inside_and_mutants_outside():
    worst, seen = {}, set()
    for c in K.adamw_cases():
        p, g, m, v = K.adamw_data(c["n"], c["seed"])
        limit = K.adamw_limit(c, g)
        R = K.adamw_ref64(p, g, m, v, c["step"], limit=limit, wd=c["wd"], **K.ADAMW_HYPER)
        ep, em, ev, en = K.adamw_emul32(p, g, m, v, c["step"], limit=limit, wd=c["wd"], **K.ADAMW_HYPER)
        for name, got in (("p", ep), ("m", em), ("v", ev), ("norm", en)):
            _check("adamw", (c, name), got, R[name], R[name + "_bound"], worst)
        for mu in K.MUTANTS["adamw"]:
            if (mu == "no_clip" and c["clip"] != "active") or (mu == "bias_step_minus_one" and c["step"] == 1):
                continue
            M = K.adamw_ref64(p, g, m, v, c["step"], limit=limit, wd=c["wd"], mutant=mu, **K.ADAMW_HYPER)
            assert max(K.ratio(ep, M["p"], R["p_bound"]), K.ratio(em, M["m"], R["m_bound"])) > 1.0, (mu, c)
            seen.add(mu)
    assert seen == set(K.MUTANTS["adamw"])
    print("AdamW emulation: max err/bound %.3f" % worst["adamw"])


def _rope_table(hd):
    from tests import stage2_ref as R

    cos, sin, _, _ = R.rope_table_hf(K.ROPE_T, hd, 10000.0)
    return cos, sin


def test_forward_sweep_emulation_inside_and_mutants_outside():
    worst, seen = {}, set()
    for c in K.rope_fwd_cases():
        n, nq, nk, hd, r, s = c["n"], c["nq"], c["nk"], c["hd"], c["r"], c["s"]
        cos, sin = _rope_table(hd)
        pos = K.rope_positions(n)
        qkv, t, bq_t, bv_t, tk, bk_t, norm = K.rope_fwd_data(c)
        ref, bound, xs, xsb = K.rope_fwd_ref64(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk, bk_t, norm)
        em, exs = K.rope_fwd_emul32(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk, bk_t, norm)
        _check("rope_fwd", c, em, ref, bound, worst)
        if norm:
            _check("rope_fwd", (c, "xsave"), exs, xs, xsb, worst)
        qk = (nq + nk) * hd
        assert K.ratio(em[:, qk:], ref[:, qk:], bound[:, qk:]) <= 1.0      # v: the delta alone, not rotated
        if n == 9:
            for m in K.MUTANTS["rope_fwd"]:
                if m == "norm_before_delta" and not norm:
                    continue
                mref = K.rope_fwd_ref64(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk, bk_t, norm, mutant=m)[0]
                _mutant_outside("rope_fwd", m, em, mref, bound, c)
                seen.add(m)
    assert seen == set(K.MUTANTS["rope_fwd"])
    print("forward sweep emulation: max err/bound %.3f" % worst["rope_fwd"])


def test_rotation_backward_is_the_adjoint_of_the_forward_rotation():
    from tests import stage2_ref as R

    for nq, nk, hd in K.ROPE_SHAPES:
        cos, sin = _rope_table(hd)
        n, heads = 9, nq + nk
        pos = K.rope_positions(n)
        x, y = K.operands("random", 1, (n, heads * hd)), K.operands("random", 2, (n, heads * hd))
        ref, bound = K.rope_bwd_ref64(y, heads, hd, pos, cos, sin)
        assert K.ratio(K.rope_bwd_emul32(y, heads, hd, pos, cos, sin), ref, bound) <= 1.0
        assert K.ratio(K.rope_bwd_emul32(y, heads, hd, pos, cos, sin), K.rope_bwd_ref64(y, heads, hd, pos, cos, sin, "forward_rotation")[0],
                       bound) > 1.0
        fwd = R.rope_rotate64(x.astype(np.float64).reshape(n, heads, hd), pos, cos, sin).reshape(n, -1)
        assert abs((fwd * y).sum() - (x * ref).sum()) < 1e-9 * np.abs(x * ref).sum()      # <R x, y> = <x, R^T y>


def test_swiglu_with_adapters_emulation_inside_and_mutant_outside():
    from tests.test_gpu_stage2_bounds import gated_ratio

    for n in K.SWIGLU_NS:
        for f in (16, 48, 2064):
            for r in (4, 16):
                g, u, t, w = K.swiglu_lora_data(n, f, r, seed=n + f + r)
                g1, u1, Dg, Du = K.swiglu_lora_ref64(g, u, t, w, r, 1.4285714)
                eg, eu, eh = K.swiglu_lora_emul32(g, u, t, w, r, 1.4285714)
                assert K.ratio(eg, g1, Dg + K.TINY) <= 1.0 and K.ratio(eu, u1, Du + K.TINY) <= 1.0
                D = K.interleave_gu(Dg.astype(np.float32), Du.astype(np.float32)).astype(np.float64)
                gu1 = K.interleave_gu(g1.astype(np.float32), u1.astype(np.float32)).astype(np.float64)
                assert gated_ratio(2, gu1, D * 2.0 ** 24, 1, eh) <= 1.0
                mg, mu, _, _ = K.swiglu_lora_ref64(g, u, t, w, r, 1.4285714, mutant="gate_up_ranks_swapped")
                assert max(K.ratio(eg, mg, Dg + K.TINY), K.ratio(eu, mu, Du + K.TINY)) > 1.0


def test_working_copy_references_place_every_element_once():
    a, b = K.hash_uniform(1, (8, 40), 0.1), K.hash_uniform(2, (192, 8), 0.1)
    a_cat, bq_t, bv_t = K.prep_lora_ref(a, b, a * 2, b[:96] * 3, 8, 96)
    assert not a_cat[8:16].any() and not a_cat[24:].any() and not bq_t[8:].any() and not bv_t[8:].any()
    # packed column 2i of a head holds HF row i, 2i + 1 HF row i + hd / 2
    assert np.array_equal(bq_t[:8, 0:96:2], K.bf16_round(b)[:48].T) and np.array_equal(bq_t[:8, 1:96:2], K.bf16_round(b)[48:96].T)
    before = np.full((16, 96), 7.0, np.float32)
    for perm, lo in ((2, 0), (3, 16)):
        _, b_t = K.prep_module_ref(a, b[:48], 8, perm, 0, before)
        written = ((np.arange(96) // 16) % 2) == (perm == 3)
        assert (b_t[:, ~written] == 7.0).all() and not b_t[8:, written].any()
        assert np.array_equal(b_t[:8, written], K.bf16_round(b[:48]).T)
