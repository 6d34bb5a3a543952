"""GPU: the stage-2 kernels against the float64 references of tests/stage2_ref.py, element by element within an error
bound derived from each kernel's rounding points (see that module's docstring) -- attention variants 1-4 and auto through
every stand-alone entry point, the GEMM epilogues at model widths, the RoPE table -- and the host-side validation of
cu_seqlens_host. Every bound test prints max(err / bound) and shows on its own data that a mutant of the reference (one
plausible kernel bug) exceeds the bound."""
import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, f32_to_bf16_bits, hash_uniform
from tests import stage2_ref as R

pytestmark = pytest.mark.gpu

LR_EINVAL = -1
EDGE = [1, 63, 64, 65, 128, 129, 256, 257, 300, 600, 1125]
REGIMES = ("flat", "peaked", "large_v", "last_block")


def _dev_bf16(x):
    return torch.from_numpy(f32_to_bf16_bits(x).view(np.int16)).cuda()


def _host(t):
    return bf16_bits_to_f32(t.cpu().numpy().view(np.uint16))


def _attn(qkv_d, cu, n, nh, nkv, hd, api, variant, want_lse):
    """One stand-alone attention call on NaN-poisoned outputs: (rc, out, lse or None)."""
    from llamarec_amd._lib import lib, stream_ptr

    L = lib()
    cu = np.ascontiguousarray(cu, dtype=np.int32)
    cud = torch.from_numpy(cu).cuda()
    B = len(cu) - 1
    out = torch.full((n, nh * hd), 0x7FC0, dtype=torch.int16, device="cuda")
    lse = torch.full((n, nh), float("nan"), dtype=torch.float32, device="cuda") if want_lse else None
    lp = lse.data_ptr() if want_lse else None
    if api == "plain":
        rc = L.lr_attention_varlen(qkv_d.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, variant,
                                   stream_ptr())
    elif api == "ws":
        wsb = L.lr_attention_workspace_bytes(n, B, nh)
        ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
        rc = L.lr_attention_varlen_ws(qkv_d.data_ptr(), out.data_ptr(), lp, cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd,
                                      variant, ws.data_ptr(), wsb, stream_ptr())
    else:
        rc = L.lr_attention_varlen_lse(qkv_d.data_ptr(), out.data_ptr(), lp, cud.data_ptr(), cu.ctypes.data, B, nh, nkv,
                                       hd, variant, stream_ptr())
    torch.cuda.synchronize()
    return rc, _host(out), (lse.cpu().numpy() if want_lse else None)


def _mutant_check(qkv, cu, nh, nkv, hd, out, bound):
    """The diagonal-key mutant of the reference, on this test's longest segment of at most 1125 rows, exceeds the bound."""
    lens = np.diff(cu)
    b = int(np.argmax(np.where(lens <= 1125, lens, 0)))
    s0, e0 = int(cu[b]), int(cu[b + 1])
    mo, _, _, _ = R.attention_ref64(qkv[s0:e0], np.array([0, e0 - s0]), nh, nkv, hd, "diag")
    r = R.ratio(mo, out[s0:e0], bound[s0:e0])
    print(f"  reference mutant 'diag': {r:.1f} x bound")
    assert r > 1.0, r


# (api, variant, lse): every way the head_dim-128 / -256 / generic kernels are reached
RUNS_128 = [("plain", 2, False), ("plain", 1, False), ("plain", 0, False), ("lse", 2, True), ("lse", 1, True),
            ("lse", 0, True), ("ws", 3, True), ("ws", 3, False), ("ws", 0, True), ("ws", 2, True)]
RUNS_256 = [("plain", 4, False), ("ws", 4, False), ("plain", 0, False), ("lse", 1, True), ("ws", 1, True)]
RUNS_GENERIC = [("plain", 1, False), ("plain", 0, False), ("lse", 1, True), ("ws", 0, True)]


def _check_attention(regime, lens, nh, nkv, hd, runs, mutant=True):
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(cu[-1])
    qkv = R.attention_data(regime, cu, nh, nkv, hd)
    ref, lse_ref, bound, lse_bound = R.attention_ref64(qkv, cu, nh, nkv, hd)
    qkv_d = _dev_bf16(qkv)
    bad = []
    for api, variant, want_lse in runs:
        rc, got, lse = _attn(qkv_d, cu, n, nh, nkv, hd, api, variant, want_lse)
        assert rc == 0, (api, variant, rc)
        r = R.ratio(got, ref, bound)
        rl = R.ratio(lse, lse_ref, lse_bound) if want_lse else 0.0
        print(f"attention {regime} hd={hd} nh={nh} nkv={nkv} T<={max(lens)} {api} v{variant}: "
              f"err/bound {r:.3f}" + (f", lse {rl:.3f}" if want_lse else ""))
        if not (r <= 1.0 and rl <= 1.0):
            bad.append((api, variant, r, rl))
    if mutant:
        _mutant_check(qkv, cu, nh, nkv, hd, ref, bound)
    assert not bad, bad


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
def test_attention_hd128_within_bound(regime, nh, nkv):
    _check_attention(regime, EDGE, nh, nkv, 128, RUNS_128)


@pytest.mark.parametrize("regime", ["flat", "last_block"])
def test_attention_hd128_long_prompts_within_bound(regime):
    _check_attention(regime, [2049, 4096], 4, 1, 128, RUNS_128)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv", [(8, 1), (16, 16)])
def test_attention_hd256_within_bound(regime, nh, nkv):
    _check_attention(regime, EDGE, nh, nkv, 256, RUNS_256)


def test_attention_hd256_8192_tokens_within_bound():
    _check_attention("flat", [8192], 2, 1, 256, [("plain", 4, False), ("lse", 1, True)], mutant=False)
    _check_attention("peaked", [700], 2, 1, 256, [("plain", 4, False)])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv,hd", [(4, 2, 16), (2, 2, 64)])
def test_attention_generic_within_bound(regime, nh, nkv, hd):
    _check_attention(regime, EDGE, nh, nkv, hd, RUNS_GENERIC)


def test_attention_hd256_refuses_lse():
    """Variant 4 writes no statistics: asked for them it must fail, not return without them."""
    cu = np.array([0, 65, 130])
    qkv_d = _dev_bf16(R.attention_data("flat", cu, 2, 1, 256))
    for api in ("ws", "lse"):
        rc, _, lse = _attn(qkv_d, cu, 130, 2, 1, 256, api, 4, True)
        assert rc != 0, api


# ---------------------------------------------------------------------------------------------------------------------
# GEMM epilogues
# ---------------------------------------------------------------------------------------------------------------------
# (name, N, rot_cols, head_dim, rope positions) / (name, N): qkv and gate-up widths of the models the ranker runs
QKV_WIDTHS = [("llama2-7b", 12288, 8192, 128, 4096), ("gemma-2b", 2560, 2304, 256, 8192), ("gemma-7b", 12288, 8192, 256, 8192)]
GU_WIDTHS = [("llama2-7b", 22016), ("gemma-7b", 32768)]
MS = [1, 7, 255, 257, 517]


def _bf16_ulp(x):
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _operands(kind, M, N, K, seed):
    """exact: small integers times powers of two, so every fp32 partial sum is exact; random: unit bf16 (A) and 0.05 (B)."""
    if kind == "exact":
        A = np.round(hash_uniform(seed + M, (M, K), 2.0)) * 0.25            # integers in [-3, 3]
        B = np.round(hash_uniform(seed + N, (N, K), 3.0)) * 0.125           # integers in [-5, 5]
        A[M // 2] = 0.0                                     # a row of exact zeros (gate and up both 0)
        acc = A.astype(np.float64) @ B.astype(np.float64).T       # every partial sum < 2^24 units of 2^-5: exact in fp32
    else:
        A = bf16_round(hash_uniform(seed + M, (M, K), 1.0))
        B = bf16_round(hash_uniform(seed + N, (N, K), 0.05))
        acc = A.astype(np.float64) @ B.astype(np.float64).T
    return A, B, acc


def _epi(A_d, B_d, M, N, K, epi, variant, R_d=None, pos_d=None, cs=None, rope_positions=0, hd=0, rot_cols=0, ws=None):
    from llamarec_amd._lib import lib, stream_ptr

    n_out = N // 2 if epi in (2, 5) else N
    C = torch.full((M, n_out), 0x7FC0, dtype=torch.int16, device="cuda")
    rc = lib().lr_gemm_bf16_nt_epi(A_d.data_ptr(), B_d.data_ptr(), C.data_ptr(), R_d.data_ptr() if R_d is not None else None,
                                   M, N, K, epi, variant, pos_d.data_ptr() if pos_d is not None else None,
                                   cs.data_ptr() if cs is not None else None, rope_positions, hd, rot_cols,
                                   ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                   stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (epi, variant, rc)
    return _host(C)


def _rope_table(T, hd):
    from llamarec_amd._lib import check, lib, stream_ptr

    L = lib()
    cs = torch.full((L.lr_rope_table_bytes(T, hd) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    check(L.lr_rope_table(cs.data_ptr(), T, hd, 10000.0, stream_ptr()), "rope table")
    torch.cuda.synchronize()
    return cs


def _report(what, got, ref, tol):
    assert np.isfinite(got).all(), what
    r = float((np.abs(got.astype(np.float64) - ref) / tol).max()) if tol is not None else float(np.abs(got - ref).max())
    print(f"{what}: " + (f"err/bound {r:.3f}" if tol is not None else f"max |err| {r:g} (bit-exact expected)"))
    return r


def _K(kind, variant):
    return 2048 if (kind == "exact" and variant == 5) else 256   # split-K needs >= 32 K tiles


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("name,N,rot_cols,hd,T", QKV_WIDTHS)
def test_qkv_epilogue_store_residual_rope_within_bound(kind, name, N, rot_cols, hd, T):
    cs = _rope_table(T, hd)
    half = hd // 2
    cs_h = cs[: T * hd].view(T, half, 2).cpu().numpy()
    cos, sin = cs_h[..., 0], cs_h[..., 1]
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    bad = []
    for variant in (1, 4, 5):
        K = _K(kind, variant)
        for M in MS:
            A, B, acc = _operands(kind, M, N, K, M + N)
            A_d, B_d = _dev_bf16(A), _dev_bf16(B)
            Rr = bf16_round(hash_uniform(M * 3 + 1, (M, N), 4.0))
            pos = ((np.arange(M) * 2654435761) % T).astype(np.int32)
            pos[0] = T - 1
            pos_d = torch.from_numpy(pos).cuda()
            if kind == "exact":
                tol_store = None
            else:
                absum = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T
                acc_err = K * 2.0 ** -24 * absum                 # fp32 accumulation over K terms
                tol_store = _bf16_ulp(acc) + acc_err
            w = ws if variant == 5 else None
            tag = f"{name} {kind} M={M} v{variant}"
            got = _epi(A_d, B_d, M, N, K, 0, variant, ws=w)
            want = R.epi_store(acc)
            r = _report(f"store {tag}", got, want if kind == "exact" else acc, tol_store)
            if (kind == "exact" and not np.array_equal(got, want)) or (kind != "exact" and r > 1):
                bad.append(("store", tag, r))
            got = _epi(A_d, B_d, M, N, K, 1, variant, R_d=_dev_bf16(Rr), ws=w)
            want = R.epi_residual(acc, Rr)
            if kind == "exact":
                r = _report(f"residual {tag}", got, want, None)
                if not np.array_equal(got, want):
                    bad.append(("residual", tag, r))
            else:   # bf16(bf16(acc) + R): acc's error may move bf16(acc) one ulp, then the sum rounds once more
                tol = _bf16_ulp(acc) + acc_err + _bf16_ulp(want)
                r = _report(f"residual {tag}", got, bf16_round(acc.astype(np.float32)) + Rr, tol)
                if r > 1:
                    bad.append(("residual", tag, r))
            for rope_positions in ((T, 0) if hd == 128 else (T,)):   # packed-table (LDS) path and float-table path
                got = _epi(A_d, B_d, M, N, K, 3, variant, pos_d=pos_d, cs=cs, rope_positions=rope_positions, hd=hd,
                           rot_cols=rot_cols, ws=w)
                want = R.epi_rope(acc, pos, cos, sin, hd, rot_cols)
                if kind == "exact":
                    r = _report(f"rope({rope_positions}) {tag}", got, want, None)
                    if not np.array_equal(got, want):
                        bad.append(("rope", rope_positions, tag, r))
                    if variant == 1 and M == 517:
                        for m in R.ROPE_MUTANTS:
                            mut = R.epi_rope(acc, pos, cos, sin, hd, rot_cols, m)
                            assert (mut != got).mean() > 0.1, m
                else:
                    # x = bf16(acc) may sit one ulp off; the rotation of |x| <= X moves by <= 2 ulp(X) (|c|, |s| <= 1)
                    x_ulp = _bf16_ulp(acc) + acc_err
                    pair = 2 * np.maximum(x_ulp, np.maximum(np.roll(x_ulp, -1, axis=1), np.roll(x_ulp, 1, axis=1))) + _bf16_ulp(want)
                    r = _report(f"rope({rope_positions}) {tag}", got, want, pair)
                    if r > 1:
                        bad.append(("rope", rope_positions, tag, r))
    assert not bad, bad[:10]


def gated_ratio(epi, acc, absum, K, got):
    """max err / bound of a SwiGLU (2) / GeGLU (5) epilogue output `got` [M][N/2] against the float64 reference.
    The reference is evaluated at the four corners (gate -, +) x (up -, +) of each accumulator's fp32 accumulation error
    K 2^-24 sum|a||b| (0 for exact operands), which covers a flip of bf16(gate) or bf16(up). The kernel's activation
    (approximate __expf / rcp / tanhf) may round to the bf16 neighbour of the reference's a = bf16(act): 1 ulp there is
    ulp(a) |u| in the output, and the output's own rounding may differ by ulp(out). GeGLU adds the fp32 tanhf's absolute
    error (<= 2^-21 near +-1) that the cancellation in 1 + tanh carries into 0.5 g (1 + t) u. 1e-30: results the
    approximate rcp / exp flush to zero."""
    d = K * 2.0 ** -24 * absum
    N = acc.shape[1]
    gate_cols = (np.arange(N) // 16) % 2 == 0
    fn, act = (R.epi_swiglu, "silu") if epi == 2 else (R.epi_geglu, "gelu")
    outs, slack = [], []
    for sg in (-1, 1):
        for su in (-1, 1):
            x = acc + np.where(gate_cols, sg, su)[None, :] * d
            outs.append(fn(x))
            a, u = R.gated_parts(x, act)
            g, _ = R._gate_up(x)
            slack.append(_bf16_ulp(a) * np.abs(u) + (0.5 * np.abs(g) * 2.0 ** -21 * np.abs(u) if epi == 5 else 0.0))
    outs, slack = np.stack(outs), np.stack(slack).max(0)
    lo, hi = outs.min(0), outs.max(0)
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    over = np.maximum((lo - got) / (_bf16_ulp(lo) + slack + 1e-30), (got - hi) / (_bf16_ulp(hi) + slack + 1e-30))
    return max(float(over.max()), 0.0)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("name,N", GU_WIDTHS)
def test_gated_epilogues_within_one_ulp(kind, name, N):
    """SwiGLU (2) and GeGLU (5): within 1 bf16 ulp at the activation's rounding point (approximate __expf / rcp / tanhf) of
    the float64 reference (gated_ratio); gate values beyond +-100 and exact zeros; every output finite."""
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    bad = []
    for variant in (1, 4, 5):
        K = _K(kind, variant)
        for M in MS:
            A, B, acc = _operands(kind, M, N, K, M + 7)
            if kind == "exact":
                B[32:48] = 0.0                                   # gate group 1: exact zeros with a live up half
                B[0:16] *= 32.0                                  # gate group 0: gates spanning +-100 and beyond
                acc = A.astype(np.float64) @ B.astype(np.float64).T
                absum = np.zeros_like(acc)
            else:
                absum = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T
            A_d, B_d = _dev_bf16(A), _dev_bf16(B)
            for epi, fn in ((2, R.epi_swiglu), (5, R.epi_geglu)):
                got = _epi(A_d, B_d, M, N, K, epi, variant, ws=ws if variant == 5 else None)
                r = gated_ratio(epi, acc, absum, K, got)
                print(f"{'swiglu' if epi == 2 else 'geglu'} {name} {kind} M={M} v{variant}: err/bound {r:.3f} "
                      f"(|gate| max {np.abs(acc[:, :16]).max():.0f})")
                if not r <= 1.0:
                    bad.append((epi, variant, M, r))
                if variant == 1 and M == 517:
                    mut = fn(acc, swap=True)
                    assert (np.abs(mut - got) > _bf16_ulp(got)).mean() > 0.3, "the swapped-halves mutant is not caught"
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------------------------------
# RoPE table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,T", [(128, 4096), (256, 8192)])
def test_rope_table_within_hf_band(hd, T):
    cs = _rope_table(T, hd)
    half = hd // 2
    f = cs[: T * hd].view(T, half, 2).cpu().numpy()
    packed = cs[T * hd:].view(torch.int32).cpu().numpy().view(np.uint32).reshape(T, half)
    cos, sin = f[..., 0], f[..., 1]
    clo, chi, slo, shi = R.rope_band(T, hd, 1e4)
    out = ~((cos >= clo) & (cos <= chi) & (sin >= slo) & (sin <= shi))
    hc, hs, _, _ = R.rope_table_hf(T, hd, 1e4)
    print(f"rope table hd={hd} T={T}: {int(out.sum())} entries outside the band, "
          f"{int(((cos != hc) | (sin != hs)).sum())} differ from HF's fp32 table")
    assert not out.any(), np.argwhere(out)[:10]
    # the packed half holds the same bf16 values: cos in the low half-word, sin in the high one
    assert np.array_equal(packed & 0xFFFF, cos.view(np.uint32) >> 16)
    assert np.array_equal(packed >> 16, sin.view(np.uint32) >> 16)
    assert np.array_equal(cos.view(np.uint32) & 0xFFFF, np.zeros_like(packed))


# ---------------------------------------------------------------------------------------------------------------------
# cu_seqlens_host validation (checked on the host: nothing is launched, the outputs stay as they were)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu", [[0, 5, 5, 12], [1, 5, 12], [0, 7, 5, 12]], ids=["empty", "nonzero_start", "decreasing"])
def test_attention_entry_points_reject_bad_segments(cu):
    from llamarec_amd._lib import lib, stream_ptr

    L = lib()
    nh = nkv = 2
    hd, n = 128, 16
    cu = np.ascontiguousarray(cu, dtype=np.int32)
    B = len(cu) - 1
    cud = torch.from_numpy(cu).cuda()
    qkv = _dev_bf16(bf16_round(hash_uniform(1, (n, (nh + 2 * nkv) * hd), 1.0)))
    out = torch.full((n, nh * hd), 0x1234, dtype=torch.int16, device="cuda")
    lse = torch.full((n, nh), 7.0, dtype=torch.float32, device="cuda")
    dqkv = torch.full_like(qkv, 0x1234)
    wsb = L.lr_attention_workspace_bytes(n, B, nh)
    ws = torch.zeros(max(wsb, 1 << 16), dtype=torch.uint8, device="cuda")
    sb = L.lr_attention_bwd_scratch_bytes(n, nh, nkv, hd)
    scratch = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    o0, l0, d0 = out.clone(), lse.clone(), dqkv.clone()
    s = stream_ptr()
    calls = {
        "varlen": lambda: L.lr_attention_varlen(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv,
                                                hd, 2, s),
        "ws": lambda: L.lr_attention_varlen_ws(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu.ctypes.data,
                                               B, nh, nkv, hd, 3, ws.data_ptr(), ws.numel(), s),
        "ws_auto": lambda: L.lr_attention_varlen_ws(qkv.data_ptr(), out.data_ptr(), None, cud.data_ptr(), cu.ctypes.data, B,
                                                    nh, nkv, hd, 0, None, 0, s),
        "lse": lambda: L.lr_attention_varlen_lse(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(),
                                                 cu.ctypes.data, B, nh, nkv, hd, 1, s),
        "bwd": lambda: L.lr_attention_varlen_bwd(qkv.data_ptr(), out.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                 dqkv.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, 2,
                                                 scratch.data_ptr(), sb, s),
        "bwd_ex": lambda: L.lr_attention_varlen_bwd_ex(qkv.data_ptr(), out.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                       dqkv.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, 1,
                                                       scratch.data_ptr(), sb, None, None, 0, 1, s),
    }
    for name, call in calls.items():
        rc = call()
        torch.cuda.synchronize()
        assert rc == LR_EINVAL, (name, rc)
        assert b"cu_seqlens" in L.lr_last_error(), (name, L.lr_last_error())
    assert torch.equal(out, o0) and torch.equal(lse, l0) and torch.equal(dqkv, d0)
