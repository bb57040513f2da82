"""Operator-level tests of the first-generation prefill GEMM (gemm.hip, the GEMM every int8
engine prefills through), one launch form at a time through the test hook llmi_debug_gemm1: the
fp32 activations, the weights (fp16, or int8 with fp16 row scales) and gamma are fed directly.
Every case first asserts, through llmi_debug_gemm1_plan, the form it names: the row tile (BM 64
or 128), the workgroups, and whether the XCD remap is on (workgroups % 8 == 0).

Sections and bars, and where each bar comes from:
  A  integer data (x in [-4, 4], W in [-3, 3] as fp16 or as int8 with power-of-two row scales
     2^-2 .. 2^2, no two neighbouring rows and no two rows 16, 32, 64 or 128 apart sharing one):
     every product, sum and scaling is exact in fp32 whatever the order (|sum| <= 4 x 3 x 320),
     the lo plane is all zeros, so y is BITWISE the exact matmul (float64 of these integers is
     exact) with split 1 and with split 2; add: bitwise y0 + matmul, y0 small integers.
  B  real data (x normal; W fp16 N(0, 1/k), or the synthetic int8 weights with their fp16 row
     scales) against float64 of the operation: the MAXIMUM OVER ROWS of the row's rel-L2 < 2e-6,
     the project's GEMM bar. Split 1 against float64 of fp16(x) W^T, the plane it multiplies.
  C  fused RMSNorm (store and gate_up; gamma fp16 and fp32): row i of x scaled by 2^(i mod 5),
     so a row that picks up another row's rstd is off by a factor >= 2; one row all zeros, whose
     output must be exactly 0; ragged m. Float64 RMSNorm, then the matmul: 2e-6 per row. Split 1
     against the plane fp16(fp32 x * fp32 gamma).
  D  gate_up on integers: gamma all ones and every x row a permutation of one multiset, so rstd
     is one known float; gate rows in [-3, 3] (every 8th x 32, so that gate passes -89, where
     expf overflows and the product is -0 x up), up rows in [0, 3]; fp16 W = gate / 4, up / 32,
     int8 W with gate scales from 2^-3 .. 2^-1 and up scales from 2^-6 .. 2^-4. y per-row rel-L2
     < 2e-6 against float64 silu(g) u of the exact g, u; the numpy fp32 restatement is held to
     the same bar on the same inputs, so the bar is not taken from the kernel.
  E  the range of "fp32-faithful": x scaled by 2^e, split 2, against float64 x W^T of the
     unsplit x: <= max(2e-6, 2 x the error of the numpy model of the planes hi = fp16(x),
     lo = fp16(x - hi)), the model computed here and printed (the factor covers the fp32
     accumulation the model does not round; the convention of test_mfma_p2_range_sweep).
  F  llmi_linear's launches bitwise the hook's; two identical launches bitwise; every refusal
     of gemm_plan through both hooks with the output untouched.
Outputs and A follow tests/test_gpu_prefill_gemm.py: 64 sentinels behind the end, ldy = n + 8,
two spare rows, a NaN start; A has lda = k + 8 with NaN padding.

Measured on an MI355X: A and F bitwise; B max row 2.0e-7 (split 1 against its plane 1.4e-7); C
5.4e-7 (split 1: 4.1e-7); D 1.2e-7, the numpy restatement's own figure; E kernel / model 3.7e-7 /
5.8e-8 at 2^0, 4, 12 (the kernel's floor is its fp32 accumulation over k = 1024), 4.0e-7 / 1.8e-7
at 2^-3, 7.1e-7 / 6.4e-7 at 2^-5, 2.74e-6 / 2.74e-6 at 2^-7, 1.03e-5 / 1.03e-5 at 2^-9 (the MFMA
multiplies fp16 subnormals: the kernel follows the model), split 1 2.63e-4 / 2.63e-4. No defect
found in gemm_kernel. Each of these breaks of the kernel fails named cases here: scales[n + 1]
(test_a_store[*-i8] and more), no pair_off in the up scale (test_d_gate_up[*-i8]),
rs_lds[lr ^ 16] (test_c_fused_rmsnorm), the remap without its (id & 7) * (nwg >> 3) term
(test_a_forms[*-True-*]), a_lo staged from hi (test_a_store, split 2).

Not covered: w_kblock != 0 (not reachable from any caller, not exposed by the hook)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import prng  # noqa: E402
from test_gpu_prefill_gemm import BAR, Out, Run, T, mm, ops, padded, report, row_err, same_bits  # noqa: E402,F401

STORE, ADD, SILU = 0, 1, 2
EPS = 1e-5
WTS = ["f16", "i8"]


def plan_model(m, n, k, epi):
    """gemm.hip's rule restated (as tests/test_lib_cpu.py): (bm, workgroups)."""
    nt = (n // 2) // 64 if epi == SILU else n // 128
    bm = 128 if -(-m // 128) * nt >= 256 else 64
    return bm, -(-m // bm) * nt


def run(ops, m, n, k, x, w, scales=None, gamma=None, split=2, epi=STORE, y0=None, form=None, launches=1, lda=None):
    """llmi_debug_gemm1 on fresh device copies. x fp32 [m, k]; w fp16 or int8 [n, k] (int8: scales
    fp16 [n]); gamma fp16 / fp32 [k] or None. form: the (bm, workgroups, remap) the case names
    (None: BM 64). Returns the read-back logical output(s), padding and sentinels checked."""
    lda = lda or k + 8
    n_out = n // 2 if epi == SILU else n
    ldy = n_out + 8
    keep = [T(padded(np.asarray(x, np.float32), lda, np.float32(np.nan))), T(w)]
    a = dict(a=keep[0], lda=lda, w=keep[1], w_dtype=_lib.I8 if w.dtype == np.int8 else _lib.F16, m=m, n=n, k=k,
             split=split, epi=epi, ldy=ldy, eps=EPS)
    assert w.dtype in (np.int8, np.float16) and (scales is not None) == (w.dtype == np.int8)
    if scales is not None:
        keep.append(T(np.asarray(scales, np.float16)))
        a["scales"] = keep[-1]
    if gamma is not None:
        keep.append(T(gamma))
        a.update(gamma=keep[-1], g_dtype=_lib.F32 if gamma.dtype == np.float32 else _lib.F16)
    y = Out(m + 2, ldy, m, n_out, y0=y0)
    a["y"] = y.t
    r = Run()
    r.plan = ops.debug_gemm1_plan(**a)
    assert r.plan == plan_model(m, n, k, epi), (r.plan, m, n, k, epi)
    if form is None:
        assert r.plan[0] == 64, r.plan
    else:
        assert r.plan == form[:2] and (r.plan[1] % 8 == 0) == form[2], (r.plan, form)
    r.reads = []
    for i in range(launches):
        if i:
            y.refill()
            if y0 is not None:
                y.t[:(m + 2) * ldy].view(m + 2, ldy)[:m, :n_out] = T(y0)
        ops.debug_gemm1(**a)
        r.reads.append(y.read())
    r.y = r.reads[0]
    return r


def pow2_scales(n, lo, hi, shift=0):
    """fp16 2^e, e in [lo, hi] (3 or 5 values): row r and rows r + 1, 16, 32, 64, 128 all differ."""
    r = np.arange(n)
    e = (r + r // 16 + shift) % (hi - lo + 1) + lo
    for d in (1, 16, 32, 64, 128):
        assert (e[d:] != e[:-d]).all()
    return (2.0 ** e).astype(np.float16)


# ------------------------------------------------------------------ A. integer data, bitwise
@functools.lru_cache(maxsize=None)
def int_case(m, n, k):
    rng = np.random.default_rng([21, m, n, k])
    c = Run()
    c.x = rng.integers(-4, 5, (m, k)).astype(np.float32)
    c.w = rng.integers(-3, 4, (n, k)).astype(np.int8)
    c.s = pow2_scales(n, -2, 2, shift=m)
    c.y0 = rng.integers(-1000, 1001, (m, n)).astype(np.float32)
    c.want = {"f16": mm(c.x, c.w), "i8": mm(c.x, c.w) * c.s.astype(np.float64)[None, :]}
    return c


def int_run(ops, m, n, k, wt, **kw):
    c = int_case(m, n, k)
    if wt == "i8":
        return run(ops, m, n, k, c.x, c.w, scales=c.s, **kw)
    return run(ops, m, n, k, c.x, c.w.astype(np.float16), **kw)


A_M, A_N, A_K = (1, 63, 64, 65, 130), (128, 256, 384), (64, 128, 192, 320)
A_SMALL = [(m, A_N[(i + j) % 3], k) for i, m in enumerate(A_M) for j, k in enumerate(A_K)]
# (m, n, k, bm, workgroups, remap)
A_FORMS = [(129, 16384, 64, 128, 256, True), (257, 11008, 64, 128, 258, False), (64, 1024, 128, 64, 8, True),
           (65, 384, 128, 64, 6, False)]


@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("m,n,k", A_SMALL)
def test_a_store(ops, m, n, k, wt):
    """BM 64: KT = 1, 2, 3, 5 against every m (ragged and clamped rows) and 1, 2, 3 column tiles."""
    want = int_case(m, n, k).want[wt].astype(np.float32)
    for split in (1, 2):
        same_bits(int_run(ops, m, n, k, wt, split=split).y, want, f"y, split {split}")


@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("m,n,k,bm,grid,remap", A_FORMS)
def test_a_forms(ops, m, n, k, bm, grid, remap, wt):
    """Both row tiles, each with the XCD remap (workgroups % 8 == 0) and with the identity order."""
    want = int_case(m, n, k).want[wt].astype(np.float32)
    for split in (1, 2):
        same_bits(int_run(ops, m, n, k, wt, split=split, form=(bm, grid, remap)).y, want, f"y, split {split}")


@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("m,n,k,form", [(65, 256, 192, None), (130, 128, 64, None), (129, 16384, 64, (128, 256, True))])
def test_a_add(ops, m, n, k, form, wt):
    c = int_case(m, n, k)
    want = (c.y0 + c.want[wt]).astype(np.float32)
    for split in (1, 2):
        same_bits(int_run(ops, m, n, k, wt, split=split, epi=ADD, y0=c.y0, form=form).y, want, f"y0 + x w^T, split {split}")


# ------------------------------------------------------------------ B. real data against float64
@functools.lru_cache(maxsize=None)
def real_case(m, n, k):
    rng = np.random.default_rng([22, m, n, k])
    c = Run()
    c.x = rng.standard_normal((m, k)).astype(np.float32)
    c.y0 = rng.standard_normal((m, n)).astype(np.float32)
    tid = prng.layer_tid(0, prng.KIND_GATE)
    c.w = {"f16": (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float16), "i8": prng.int8_weight(3, tid, n, k)}
    c.s = {"f16": None, "i8": prng.int8_row_scale(3, tid, n)}
    c.w64 = {"f16": c.w["f16"].astype(np.float64),
             "i8": c.w["i8"].astype(np.float64) * c.s["i8"].astype(np.float64)[:, None]}
    return c


B_SHAPES = [(130, 256, 320, None), (129, 16384, 128, (128, 256, True))]


@pytest.mark.parametrize("split", [2, 1])
@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("epi", [STORE, ADD])
@pytest.mark.parametrize("m,n,k,form", B_SHAPES)
def test_b_real_against_float64(ops, m, n, k, form, epi, wt, split):
    c = real_case(m, n, k)
    r = run(ops, m, n, k, c.x, c.w[wt], scales=c.s[wt], split=split, epi=epi, y0=c.y0 if epi == ADD else None, form=form)
    plane = c.x if split == 2 else c.x.astype(np.float16)
    ref = plane.astype(np.float64) @ c.w64[wt].T + (c.y0.astype(np.float64) if epi == ADD else 0.0)
    e = row_err(r.y, ref)
    report("B", f"gemm1 {wt} split {split} epi {epi} ({m}, {n}, {k}) max row", e)
    assert e < BAR


# ------------------------------------------------------------------ C. the fused RMSNorm
@functools.lru_cache(maxsize=None)
def norm_case(m, n, k):
    rng = np.random.default_rng([23, m, n, k])
    c = real_case(m, n, k)
    d = Run()
    d.zero = min(m - 1, 37)
    d.x = (rng.standard_normal((m, k)) * (2.0 ** (np.arange(m) % 5))[:, None]).astype(np.float32)
    d.x[d.zero] = 0.0
    g = 1.0 + 0.1 * rng.standard_normal(k)
    d.gamma = {"f16": g.astype(np.float16), "f32": g.astype(np.float32)}
    d.rstd = 1.0 / np.sqrt((d.x.astype(np.float64) ** 2).mean(axis=1) + EPS)
    d.w, d.s, d.w64 = c.w, c.s, c.w64
    return d


def silu64(g, u):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * u


C_CASES = [(STORE, 130, 256, 320, None), (STORE, 257, 11008, 192, (128, 258, False)),
           (SILU, 130, 2 * 128, 320, None), (SILU, 129, 2 * 8192, 192, (128, 256, True))]


@pytest.mark.parametrize("split", [2, 1])
@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("gt", ["f16", "f32"])
@pytest.mark.parametrize("epi,m,n,k,form", C_CASES)
def test_c_fused_rmsnorm(ops, epi, m, n, k, form, gt, wt, split):
    d = norm_case(m, n, k)
    gam = d.gamma[gt]
    r = run(ops, m, n, k, d.x, d.w[wt], scales=d.s[wt], gamma=gam, split=split, epi=epi, form=form)
    if split == 2:
        plane = d.x.astype(np.float64) * gam.astype(np.float64)
    else:
        plane = (d.x * gam.astype(np.float32)).astype(np.float16).astype(np.float64)
    v = (plane @ d.w64[wt].T) * d.rstd[:, None]
    ref = silu64(v[:, :n // 2], v[:, n // 2:]) if epi == SILU else v
    assert (r.y[d.zero] == 0).all(), "the all-zero row"
    e = row_err(r.y, ref)
    report("C", f"gemm1 {wt} gamma {gt} split {split} epi {epi} ({m}, {n}, {k}) max row", e)
    assert e < BAR


# ------------------------------------------------------------------ D. gate_up on integers
@functools.lru_cache(maxsize=None)
def silu_case(m, inter, k):
    rng = np.random.default_rng([24, m, inter, k])
    c = Run()
    base = rng.integers(-4, 5, k)
    c.x = np.stack([rng.permutation(base) for _ in range(m)]).astype(np.float32)
    ss = np.float32((base * base).sum())                     # exact, every row's
    c.rstd = np.float32(1) / np.sqrt(ss / np.float32(k) + np.float32(EPS))
    wg = rng.integers(-3, 4, (inter, k))
    wg[::8] *= 32
    wu = rng.integers(0, 4, (inter, k))
    c.wi = np.concatenate([wg, wu]).astype(np.int8)
    c.scale = {"f16": np.concatenate([np.full(inter, 1 / 4), np.full(inter, 1 / 32)]).astype(np.float16),
               "i8": np.concatenate([pow2_scales(inter, -3, -1), pow2_scales(inter, -6, -4, shift=1)])}
    c.gamma = np.ones(k, np.float16)
    return c


D_SHAPES = [(65, 64, 128, None), (130, 128, 64, None), (1, 192, 192, None), (129, 8192, 64, (128, 256, True))]


@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("m,inter,k,form", D_SHAPES)
def test_d_gate_up(ops, m, inter, k, form, wt):
    c = silu_case(m, inter, k)
    sc = c.scale[wt].astype(np.float64)
    acc = mm(c.x, c.wi) * (sc[None, :] if wt == "f16" else 1.0)   # the accumulators: exact in fp32
    post = 1.0 if wt == "f16" else sc[None, :]                   # the epilogue's int8 row scales
    v = acc * float(c.rstd) * post
    g, u = v[:, :inter], v[:, inter:]
    assert (g < -89).any() and (g > 89).any() and np.abs(acc).max() < 2 ** 24
    ref = silu64(g, u)
    v32 = acc.astype(np.float32) * c.rstd * np.asarray(post, np.float32)
    with np.errstate(over="ignore"):
        np32 = v32[:, :inter] / (np.float32(1) + np.exp(-v32[:, :inter])) * v32[:, inter:]
    e32 = row_err(np32, ref)
    report("D", f"numpy fp32 restatement {wt} ({m}, {inter}, {k}) max row", e32)
    assert e32 < BAR
    if wt == "f16":
        w, s = (c.wi.astype(np.float64) * sc[:, None]).astype(np.float16), None
    else:
        w, s = c.wi, c.scale[wt]
    ys = []
    for split in (1, 2):
        r = run(ops, m, 2 * inter, k, c.x, w, scales=s, gamma=c.gamma, split=split, epi=SILU, form=form)
        e = row_err(r.y, ref)
        report("D", f"gemm1 {wt} gate_up split {split} ({m}, {inter}, {k}) max row", e)
        assert e < BAR
        ys.append(r.y)
    same_bits(ys[0], ys[1], "split 1 against split 2")           # integers: the lo plane is zero


# ------------------------------------------------------------------ E. the range of the two planes
E_SHAPE = (64, 128, 1024)
E_EXPS = [0, -3, -5, -7, -9, 4, 12]


@functools.lru_cache(maxsize=None)
def range_case():
    m, n, k = E_SHAPE
    rng = np.random.default_rng([25, m, n, k])
    return rng.standard_normal((m, k)).astype(np.float32), (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float16)


def planes_model(x, w, split):
    """float64 (hi [+ lo]) W^T of the numpy planes (round to nearest even, fp16 subnormals kept)."""
    hi = x.astype(np.float16)
    p = hi.astype(np.float64)
    if split == 2:
        p = p + (x - hi.astype(np.float32)).astype(np.float16).astype(np.float64)
    return p @ w.astype(np.float64).T


@pytest.mark.parametrize("e,split", [(e, 2) for e in E_EXPS] + [(0, 1)])
def test_e_range_sweep(ops, e, split):
    """The claim has a range: the lo plane is an unscaled fp16, so it sinks into subnormals as x
    shrinks. Measured figures: DESIGN.md, "First-generation GEMM, one form at a time"."""
    m, n, k = E_SHAPE
    x0, w = range_case()
    x = (x0 * np.float32(2.0 ** e)).astype(np.float32)
    full = mm(x, w)
    em = row_err(planes_model(x, w, split), full)
    r = run(ops, m, n, k, x, w, split=split)
    ek = row_err(r.y, full)
    report("E", f"x * 2^{e} split {split}: planes model max row", em)
    report("E", f"x * 2^{e} split {split}: kernel max row", ek)
    assert ek <= max(BAR, 2 * em)


# ------------------------------------------------------------------ F. plumbing
def test_f_llmi_linear_int8_launches_what_the_hook_launches(ops):
    m, n, k = 130, 256, 192
    c = real_case(m, n, k)
    y = ops.launchLinearGemm(T(c.x), T(c.w["i8"]), T(c.s["i8"]))
    torch.cuda.synchronize()
    r = run(ops, m, n, k, c.x, c.w["i8"], scales=c.s["i8"], split=2)
    same_bits(r.y, y.cpu().numpy(), "llmi_linear (int8) against the hook")


def test_f_llmi_linear_f16_below_16_rows_launches_what_the_hook_launches(ops):
    """9 <= m < 16 with fp16 weights: the one fp16 llmi_linear shape class that still runs gemm.hip."""
    m, n, k = 9, 128, 64
    c = real_case(m, n, k)
    y = ops.launchLinearGemm(T(c.x), T(c.w["f16"]))
    torch.cuda.synchronize()
    r = run(ops, m, n, k, c.x, c.w["f16"], split=2)
    same_bits(r.y, y.cpu().numpy(), "llmi_linear (fp16, m 9) against the hook")
    e = row_err(r.y, mm(c.x, c.w["f16"]))
    report("F", f"gemm1 f16 split 2 ({m}, {n}, {k}) max row", e)
    assert e < BAR


@pytest.mark.parametrize("wt", WTS)
def test_f_two_launches_are_bitwise_equal(ops, wt):
    m, n, k = 130, 256, 320
    c = real_case(m, n, k)
    r = run(ops, m, n, k, c.x, c.w[wt], scales=c.s[wt], launches=2)
    same_bits(r.reads[1], r.reads[0], "the second launch")


def test_f_refusals(ops):
    """Every LLMI_REQUIRE of gemm_plan through both hooks: LlmiError, and the output (NaN body
    and sentinels) is untouched."""
    m, n, k, lda, ldy = 64, 256, 128, 136, 264
    x = torch.zeros(m, lda, dtype=torch.float32, device="cuda")
    w = torch.zeros(n, k, dtype=torch.float16, device="cuda")
    w8 = torch.zeros(n, k, dtype=torch.int8, device="cuda")
    s = torch.ones(n, dtype=torch.float16, device="cuda")
    g16 = torch.ones(k + 8, dtype=torch.float16, device="cuda")
    g32 = torch.ones(k + 8, dtype=torch.float32, device="cuda")
    y = Out(m, ldy, 0, 0)
    Y = y.t.data_ptr()
    base = dict(a=x, lda=lda, w=w, w_dtype=_lib.F16, m=m, n=n, k=k, split=2, epi=STORE, y=Y, ldy=ldy, eps=EPS)
    gam = dict(gamma=g16, g_dtype=_lib.F16)
    silu = dict(epi=SILU, **gam)
    bad = [dict(a=None), dict(w=None), dict(y=None), dict(m=0), dict(n=192), dict(k=96), dict(lda=k - 4), dict(lda=k + 2),
           dict(a=x.data_ptr() + 8), dict(w=w.data_ptr() + 8), dict(gamma=g16.data_ptr() + 4, g_dtype=_lib.F16),
           dict(gamma=g32.data_ptr() + 8, g_dtype=_lib.F32), dict(gamma=g16, g_dtype=_lib.I8),
           dict(w=w8, w_dtype=_lib.I8), dict(w_dtype=_lib.F32), dict(split=0), dict(split=3), dict(epi=3),
           dict(epi=ADD, **gam), dict(epi=SILU), dict(silu, n=2 * 96), dict(ldy=n - 1), dict(silu, ldy=n // 2 - 1)]
    for b in bad:
        a = dict(base, **b)
        with pytest.raises(_lib.LlmiError):
            ops.debug_gemm1_plan(**a)
        with pytest.raises(_lib.LlmiError):
            ops.debug_gemm1(**a)
    # the forms the mutations start from are accepted
    for ok in (dict(), gam, dict(gamma=g32, g_dtype=_lib.F32), dict(gamma=g16.data_ptr() + 8, g_dtype=_lib.F16),
               dict(w=w8, w_dtype=_lib.I8, scales=s), dict(split=1), dict(epi=ADD), silu):
        assert ops.debug_gemm1_plan(**dict(base, **ok)) == (64, 2)
    y.read()
