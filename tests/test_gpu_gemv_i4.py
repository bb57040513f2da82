"""The int4 GEMV (LLMI_I4, gemv_i4.hip) through llmi_debug_gemv against float64 numpy on the
exactly dequantised weights (tests/i4_ref.py), at the project's GEMV bar (BAR = 2e-6 rel-L2 of
tests/test_gpu_engine_kernels.py). The three forms of a single-rank token step:
  q/k/v    x int64 fixed point + RMSNorm (fp16 gamma), EPI_STORE
  gate_up  the same input, EPI_SILU_MUL
  down     fp32 x, EPI_ATOMIC (atomic add and single producer), compared as int64 * 2^-32
K: 128 (one group, most lanes masked), 512, 1024, 4096 and 11008 (344 chunks: masked slots in the
last batch, the widest x staging); rows 2, 5 (a row tail) and 130 (more than one workgroup).
Every output buffer carries sentinels past its end and starts as NaN / garbage."""
import numpy as np
import pytest

import i4_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402

DEV = "cuda"
BAR = 2e-6  # tests/test_gpu_engine_kernels.py
PAD = 64
FX = 2.0 ** 32
STORE, ADD, SILU, ARGMAX, ATOMIC = range(5)
KS = [128, 512, 1024, 4096, 11008]
NS = [2, 5, 130]
_SENT = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buf:
    def __init__(self, n, dtype=torch.float32, init=None):
        it, self.pat = _SENT[dtype]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t = self.raw.view(dtype)
        self.n = n
        if init is not None:
            self.t[:n] = T(np.asarray(init))

    def get(self):
        torch.cuda.synchronize()
        assert (self.raw[self.n:].cpu().numpy() == self.pat).all(), "a store past the buffer's logical end"
        return self.t[:self.n].cpu().numpy().copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == self.pat).all())


def make_w(rng, n, k, scales=None, lo=-7):
    """(device args, float64 dequantised W): q uniform in [lo, 7], fp16 group scales."""
    q = rng.integers(lo, 8, (n, k)).astype(np.int8)
    if scales is None:
        scales = (0.002 + 0.002 * rng.random((n, k // 128))).astype(np.float16)
    d = dict(w=T(i4_ref.pack(q)), scales=T(scales), w_dtype=_lib.I4, n_rows=n, k=k)
    return d, i4_ref.dequant(q, scales, np.float64)


def make_gamma(rng, k):
    return (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16)


def gargs(gamma):
    return dict(gamma=T(gamma), g_dtype=_lib.F16, eps=1e-5)


def fixed_x(rng, k):
    """(int64 fixed-point x, the fp32 image the kernel stages)."""
    xf = np.rint(rng.standard_normal(k) * FX).astype(np.int64)
    return xf, xf.astype(np.float32) * np.float32(1.0 / FX)


def x_eff(x, gamma, eps=1e-5):
    x = np.asarray(x, np.float64)
    return x * gamma.astype(np.float64) / np.sqrt(np.mean(x * x) + eps)


def silu_ref(acc, po):
    g, u = acc[:po], acc[po:]
    return g / (1.0 + np.exp(-g)) * u


def run_store(ops, wa, xf, gamma, **extra):
    y, xo = Buf(wa["n_rows"]), Buf(wa["k"])
    ops.debug_gemv(**wa, x_fixed=T(xf), x_out=xo.t, y=y.t, epi=STORE, **gargs(gamma), **extra)
    return y.get(), xo.get()


def run_down(ops, wa, x, seed=None, single=False):
    n = wa["n_rows"]
    if single:
        yacc = Buf(n, torch.int64)
        ops.debug_gemv(**wa, x=T(x), epi=ATOMIC, yacc=yacc.t, yacc_single=1,
                       yacc_base=None if seed is None else T(seed))
    else:
        yacc = Buf(n, torch.int64, init=np.zeros(n, np.int64) if seed is None else seed)
        ops.debug_gemv(**wa, x=T(x), epi=ATOMIC, yacc=yacc.t)
    return yacc.get()


# ------------------------------------------------------------------ accuracy, every form
@pytest.mark.parametrize("k", KS)
def test_three_forms_against_float64(ops, k):
    rng = np.random.default_rng(k)
    gamma = make_gamma(rng, k)
    xf, x32 = fixed_x(rng, k)
    xe = x_eff(x32, gamma)
    xd = rng.standard_normal(k).astype(np.float32)
    for n in NS:
        wa, w64 = make_w(rng, n, k)
        grid, unroll, xpt = ops.debug_gemv_plan(**wa, x_fixed=T(xf), y=Buf(n).t, epi=STORE, **gargs(gamma))
        assert unroll in (2, 3, 4) and grid >= 1
        # q/k/v: store
        y, xo = run_store(ops, wa, xf, gamma)
        np.testing.assert_array_equal(xo.view(np.uint32), x32.view(np.uint32))
        r = rel(y, w64 @ xe)
        print(f"[rel-L2] i4 store k={k} rows={n} (grid {grid} unroll {unroll} xpt {xpt}): {r:.3e}")
        assert r < BAR
        # gate_up: n pairs
        w2, w2_64 = make_w(rng, 2 * n, k)
        y = Buf(n)
        ops.debug_gemv(**w2, x_fixed=T(xf), y=y.t, epi=SILU, pair_off=n, **gargs(gamma))
        r = rel(y.get(), silu_ref(w2_64 @ xe, n))
        print(f"[rel-L2] i4 silu k={k} pairs={n}: {r:.3e}")
        assert r < BAR
        # down: the atomic add onto a seed, and the single-producer store (the same integers)
        ref = w64 @ xd.astype(np.float64)
        seed = rng.integers(-2 ** 40, 2 ** 40, n)
        got = run_down(ops, wa, xd, seed)
        r = rel((got - seed) / FX, ref)
        print(f"[rel-L2] i4 atomic k={k} rows={n}: {r:.3e}")
        assert r < BAR
        np.testing.assert_array_equal(run_down(ops, wa, xd, seed, single=True), got)
        np.testing.assert_array_equal(run_down(ops, wa, xd, None, single=True), got - seed)


def test_explicit_grid_waves_loop_over_row_groups(ops):
    """grid 3 over 65 row groups: every wave loops (the later groups' loads and scales)."""
    rng = np.random.default_rng(77)
    n, k = 130, 1024
    gamma = make_gamma(rng, k)
    xf, x32 = fixed_x(rng, k)
    wa, w64 = make_w(rng, n, k)
    y, _ = run_store(ops, wa, xf, gamma, grid=3)
    r = rel(y, w64 @ x_eff(x32, gamma))
    print(f"[rel-L2] i4 store grid=3: {r:.3e}")
    assert r < BAR
    y0, _ = run_store(ops, wa, xf, gamma)
    np.testing.assert_array_equal(y.view(np.uint32), y0.view(np.uint32))


# ------------------------------------------------------------------ group-scale addressing
@pytest.mark.parametrize("form,k", [("down", 11008), ("store", 4096)])
def test_each_group_takes_its_own_scale(ops, form, k):
    """Group g has scale 2^(g mod 20 - 10); x is nonzero in one group at a time: the result is
    that group's alone. A scale taken from a neighbouring group is off by a power of two."""
    rng = np.random.default_rng(k + 1)
    n, ng = 5, k // 128
    scales = np.tile(2.0 ** ((np.arange(ng) % 20) - 10.0), (n, 1)).astype(np.float16)
    wa, w64 = make_w(rng, n, k, scales=scales)
    gamma = make_gamma(rng, k)
    worst = 0.0
    for g in range(ng):
        sl = slice(g * 128, (g + 1) * 128)
        if form == "down":
            x = np.zeros(k, np.float32)
            x[sl] = rng.standard_normal(128).astype(np.float32)
            got = run_down(ops, wa, x, None, single=True) / FX
            ref = w64[:, sl] @ x[sl].astype(np.float64)
            r = rel(got, ref)
            assert r < BAR, (g, r)
            worst = max(worst, r)
        else:
            xf = np.zeros(k, np.int64)
            xf[sl] = np.rint(rng.standard_normal(128) * FX).astype(np.int64)
            x32 = xf.astype(np.float32) * np.float32(1.0 / FX)
            y, _ = run_store(ops, wa, xf, gamma)
            xe = x_eff(x32, gamma)
            r = rel(y, w64[:, sl] @ xe[sl])
            assert r < BAR, (g, r)
            worst = max(worst, r)
    print(f"[rel-L2] i4 group scales, {form} k={k}: worst of {ng} groups {worst:.3e}")


# ------------------------------------------------------------------ nibble 0
def test_nibble_zero_decodes_as_minus_eight(ops):
    rng = np.random.default_rng(8)
    n, k = 5, 512
    # every nibble value, 0 included (the quantiser never writes it; the kernel must decode -8)
    wa, w64 = make_w(rng, n, k, lo=-8)
    b = wa["w"].cpu().numpy()
    assert (b & 0x0F == 0).any() and (b >> 4 == 0).any()
    x = rng.standard_normal(k).astype(np.float32)
    got = run_down(ops, wa, x, None, single=True) / FX
    assert rel(got, w64 @ x.astype(np.float64)) < BAR
    # a hand-packed row of nothing but nibble 0 against x = 1: -8 * sum of the group scales * 128
    scales = (2.0 ** -np.arange(1, 5, dtype=np.float64)).astype(np.float16)[None, :].repeat(2, 0)
    hand = dict(w=T(np.zeros((2, k // 2), np.uint8)), scales=T(scales), w_dtype=_lib.I4, n_rows=2, k=k)
    got = run_down(ops, hand, np.ones(k, np.float32), None, single=True) / FX
    np.testing.assert_array_equal(got, np.full(2, -8.0 * 128 * scales[0].astype(np.float64).sum()))
    gamma = np.ones(k, np.float16)
    xf = np.full(k, int(FX), np.int64)
    y, _ = run_store(ops, hand, xf, gamma)
    assert rel(y, np.full(2, -8.0 * 128 * scales[0].astype(np.float64).sum() / np.sqrt(1.0 + 1e-5))) < BAR


# ------------------------------------------------------------------ refusals
def test_unsupported_forms_launch_nothing(ops):
    rng = np.random.default_rng(9)
    n, k = 6, 512
    wa, _ = make_w(rng, n, k)
    gamma = make_gamma(rng, k)
    xf, x32 = fixed_x(rng, k)
    g16, g32 = gargs(gamma), dict(gamma=T(gamma.astype(np.float32)), g_dtype=_lib.F32, eps=1e-5)
    proj = dict(wa, x_fixed=T(xf), epi=STORE, **g16)
    down = dict(wa, x=T(x32), epi=ATOMIC)

    def refused(what, args, outs, code=-2):
        bufs = {f: Buf(m, dt) for f, (m, dt) in outs.items()}
        a = dict(args, **{f: b.t for f, b in bufs.items()})
        for fn in (ops.debug_gemv_plan, ops.debug_gemv):
            with pytest.raises(_lib.LlmiError, match=rf"\({code}\)") as ei:
                fn(**a)
            assert code != -2 or "int4" in str(ei.value), what
        assert all(b.untouched() for b in bufs.values()), f"{what}: a refused call wrote an output"

    y, yacc = dict(y=(n, torch.float32)), dict(yacc=(n, torch.int64))
    refused("kpar", dict(proj, kpar=2), y)
    refused("ldw", dict(proj, ldw=k + 128), y)
    refused("argmax", dict(proj, epi=ARGMAX), dict(y=(n, torch.float32), partials=(16, torch.int64)))
    refused("add", dict(wa, x=T(x32), epi=ADD, resid=T(np.zeros(n, np.float32))), y)
    refused("fp32 x, store", dict(wa, x=T(x32), epi=STORE), y)
    refused("fp32 x with rmsnorm", dict(wa, x=T(x32), epi=STORE, **g16), y)
    refused("fp32 gamma", dict(wa, x_fixed=T(xf), epi=SILU, pair_off=n // 2, **g32), dict(y=(n // 2, torch.float32)))
    refused("split-K", dict(down, ksplit=2), yacc)
    refused("atomic with rmsnorm", dict(down, **g16), yacc)
    # the multi-row GEMV has no int4 form
    ys = [Buf(n), Buf(n)]
    with pytest.raises(_lib.LlmiError, match=r"\(-2\).*int4"):
        ops.debug_gemv_rows([dict(proj, y=b.t) for b in ys])
    assert all(b.untouched() for b in ys)
    # argument errors stay argument errors: k not a whole group, no scales
    refused("k % 128", dict(proj, k=k - 32), y, code=-1)
    refused("no scales", {f: v for f, v in proj.items() if f != "scales"}, y, code=-1)
    # ldw == k is the dense layout
    yb = Buf(n)
    ops.debug_gemv(**dict(proj, ldw=k), y=yb.t)
    y0, _ = run_store(ops, wa, xf, gamma)
    np.testing.assert_array_equal(yb.get().view(np.uint32), y0.view(np.uint32))
