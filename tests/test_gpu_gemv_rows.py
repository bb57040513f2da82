"""The multi-row GEMV of a batched decode step (llmi_debug_gemv_rows, gemv_rows.hip) against
the single-row GEMV it must reproduce: ONE launch for m activation rows, then m launches of
llmi_debug_gemv on copies of the buffers, and every output compared BITWISE (torch.equal on
the raw bits, the int64 accumulators and the argmax keys included) -- no tolerance.

Shapes: 37 weight rows (an odd tail group, a partly filled workgroup); K with a masked chunk
tail for every weight type (fp16 536, int8 1072, fp32 268: 67 16-byte chunks), and for fp16
the 7B / 13B widths 4096, 5120 and 11008, where 8 fp32 images of x no longer fit the LDS
(11008: three images a launch). The rows get different x and every row's buffers are separate
allocations. Every output buffer carries sentinels past its end and starts as NaN / garbage."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402

DEV = "cuda"
PAD = 64
FX = 2.0 ** 32
N_ROWS = 37
PO = 19
WDT = {"f16": _lib.F16, "f32": _lib.F32, "i8": _lib.I8}
EPL = {"f16": 8, "f32": 4, "i8": 16}
K_TAIL = {"f16": 536, "i8": 1072, "f32": 268}
STORE, ADD, SILU, ARGMAX, ATOMIC = range(5)
_SENT = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buf:
    """n elements + PAD sentinels, the logical part NaN / garbage unless init is given."""

    def __init__(self, n, dtype=torch.float32, init=None):
        it, self.pat = _SENT[dtype]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t = self.raw.view(dtype)
        self.n = n
        if init is not None:
            self.t[:n] = T(np.asarray(init))

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == self.pat).all())

    def check_pad(self):
        torch.cuda.synchronize()
        assert bool((self.raw[self.n:] == self.pat).all()), "a store past the buffer's logical end"


def weights(wdt, n, k, seed):
    """W [n, k] on the device (+ per-row fp16 scales for int8), shared by the rows."""
    rng = np.random.default_rng(seed)
    d = dict(w_dtype=WDT[wdt], n_rows=n, k=k)
    if wdt == "i8":
        d["w"] = T(rng.integers(-127, 128, (n, k)).astype(np.int8))
        d["scales"] = T((0.002 + 0.001 * rng.random(n)).astype(np.float16))
    else:
        w = (0.05 * rng.standard_normal((n, k))).astype(np.float16)
        d["w"] = T(w if wdt == "f16" else w.astype(np.float32))
    return d


def gamma_args(rng, k, f16):
    g = (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16 if f16 else np.float32)
    return dict(gamma=T(g), g_dtype=_lib.F16 if f16 else _lib.F32, eps=1e-5)


def both(ops, m, common, inputs, outputs, alias=None):
    """One rows launch and m single-row launches on copies; compare every output's raw bits.
    inputs: [m] dicts field -> host array. outputs: field -> (n, dtype, [m] initial values or
    None). alias: field -> output field whose buffer it shares."""
    sets = []
    for _ in range(2):
        rows, bufs = [], []
        for i in range(m):
            d = dict(common)
            d.update({f: T(v) for f, v in inputs[i].items()})
            b = {f: Buf(n, dt, None if init is None else init[i]) for f, (n, dt, init) in outputs.items()}
            d.update({f: bb.t for f, bb in b.items()})
            for dst, src in (alias or {}).items():
                d[dst] = b[src].t
            rows.append(d)
            bufs.append(b)
        sets.append((rows, bufs))
    (rows_b, bufs_b), (rows_s, bufs_s) = sets
    ops.debug_gemv_rows(rows_b)
    for d in rows_s:
        ops.debug_gemv(**d)
    torch.cuda.synchronize()
    for i in range(m):
        for f in outputs:
            got, ref = bufs_b[i][f], bufs_s[i][f]
            got.check_pad()
            ref.check_pad()
            if outputs[f][2] is None:
                assert not bool((ref.raw[:ref.n] == ref.pat).any()), f"the single-row launch left {f} unwritten"
            assert torch.equal(got.raw, ref.raw), f"row {i} of {m}: {f} differs from the single-row launch"
    if m > 1 and "y" in outputs:  # different x per row: the rows must not be copies of one another
        assert not torch.equal(bufs_b[0]["y"].raw, bufs_b[1]["y"].raw)


def xs_fp32(rng, m, k):
    return [(rng.standard_normal(k) * (1.0 + i)).astype(np.float32) for i in range(m)]


def xs_fixed(rng, m, k):
    return [np.rint(rng.standard_normal(k) * (1.0 + 0.5 * i) * FX).astype(np.int64) for i in range(m)]


def all_forms(ops, wdt, m, k):
    rng = np.random.default_rng(1000 * m + k)
    n = N_ROWS
    W = weights(wdt, n, k, seed=k)
    W2 = weights(wdt, 2 * PO, k, seed=k + 1)
    f32 = torch.float32
    i64 = torch.int64
    # store from an fp32 x
    both(ops, m, dict(W, epi=STORE), [dict(x=x) for x in xs_fp32(rng, m, k)], dict(y=(n, f32, None)))
    # store from x_fixed with RMSNorm; x_out per row
    for f16 in (True, False):
        both(ops, m, dict(W, epi=STORE, **gamma_args(rng, k, f16)), [dict(x_fixed=x) for x in xs_fixed(rng, m, k)],
             dict(y=(n, f32, None), x_out=(k, f32, None)))
    # silu(gate) * up over the pairs (g, g + 19), fp32 x and the engine's normed fixed-point x
    both(ops, m, dict(W2, epi=SILU, pair_off=PO), [dict(x=x) for x in xs_fp32(rng, m, k)], dict(y=(PO, f32, None)))
    both(ops, m, dict(W2, epi=SILU, pair_off=PO, **gamma_args(rng, k, True)),
         [dict(x_fixed=x) for x in xs_fixed(rng, m, k)], dict(y=(PO, f32, None)))
    # add with a residual per row
    both(ops, m, dict(W, epi=ADD, resid_scale=0.75),
         [dict(x=x, resid=rng.standard_normal(n).astype(np.float32)) for x in xs_fp32(rng, m, k)],
         dict(y=(n, f32, None)))
    # argmax: logits and the per-workgroup best keys, one partials array per row
    common = dict(W, epi=ARGMAX, idx_base=32000, **gamma_args(rng, k, True))
    probe = dict(common, x_fixed=T(np.zeros(k, np.int64)), y=T(np.zeros(n, np.float32)),
                 partials=T(np.zeros(64, np.int64)))
    grid = ops.debug_gemv_plan(**probe)[0]
    both(ops, m, common, [dict(x_fixed=x) for x in xs_fixed(rng, m, k)],
         dict(y=(n, f32, None), partials=(grid, i64, None)))
    # split-K atomics (ksplit 4) onto a non-zero accumulator; K rounded up to 4 whole chunk slices
    step = 4 * EPL[wdt]
    ka = (k + step - 1) // step * step
    Wa = W if ka == k else weights(wdt, n, ka, seed=ka)
    seeds = [rng.integers(-2 ** 40, 2 ** 40, n) for _ in range(m)]
    both(ops, m, dict(Wa, epi=ATOMIC, ksplit=4), [dict(x=x) for x in xs_fp32(rng, m, ka)],
         dict(yacc=(n, i64, seeds)))
    # single producer: yacc = yacc_base + fixed(acc), the copy aliasing the base (the engine's use)
    both(ops, m, dict(W, epi=ATOMIC, yacc_single=1), [dict(x=x) for x in xs_fp32(rng, m, k)],
         dict(yacc=(n, i64, None), yacc_base=(n, i64, seeds)), alias=dict(yacc_copy="yacc_base"))
    # ... and into a separate copy, the base left alone
    both(ops, m, dict(W, epi=ATOMIC, yacc_single=1), [dict(x=x) for x in xs_fp32(rng, m, k)],
         dict(yacc=(n, i64, None), yacc_base=(n, i64, seeds), yacc_copy=(n, i64, None)))
    # the seed copy on the side (kept, and zeroed), 300 elements over the grid's slices
    for keep in (1, 0):
        both(ops, m, dict(W2, epi=SILU, pair_off=PO, seed_n=300, seed_keep=keep, **gamma_args(rng, k, True)),
             [dict(x_fixed=x, seed_src=rng.integers(-2 ** 50, 2 ** 50, 300)) for x in xs_fixed(rng, m, k)],
             dict(y=(PO, f32, None), seed_dst=(300, i64, None)))


@pytest.mark.parametrize("m", [2, 3, 8])
@pytest.mark.parametrize("wdt", ["f16", "i8", "f32"])
def test_rows_every_form_masked_chunk_tail(ops, wdt, m):
    """67 chunks a row: one partly filled batch, lanes 3 .. 63 of its second load masked."""
    all_forms(ops, wdt, m, K_TAIL[wdt])


@pytest.mark.parametrize("m", [2, 3, 8])
@pytest.mark.parametrize("k", [4096, 5120, 11008])
def test_rows_every_form_fp16_model_widths(ops, k, m):
    """The staging widths of the single-row kernel (4, 5, 11 float4s a thread) and, at m = 8, the
    LDS limit: 4096 fills it with one workgroup per CU, 5120 and 11008 overflow it and run as
    several launches (4 + 4, and 3 + 3 + 2)."""
    all_forms(ops, "f16", m, k)


@pytest.mark.parametrize("m", [4, 5, 6, 7])
def test_rows_other_row_counts(ops, m):
    """The instantiations between the ones above, store / argmax / single-producer forms."""
    rng = np.random.default_rng(m)
    k, n = 536, N_ROWS
    W = weights("f16", n, k, seed=3)
    both(ops, m, dict(W, epi=STORE, **gamma_args(rng, k, True)), [dict(x_fixed=x) for x in xs_fixed(rng, m, k)],
         dict(y=(n, torch.float32, None), x_out=(k, torch.float32, None)))
    both(ops, m, dict(W, epi=ATOMIC, yacc_single=1), [dict(x=x) for x in xs_fp32(rng, m, k)],
         dict(yacc=(n, torch.int64, None)))


def test_rows_argument_checks_launch_nothing(ops):
    rng = np.random.default_rng(5)
    k, n = 536, N_ROWS
    W = weights("f16", n, k, seed=4)
    W_other = weights("f16", n, k, seed=6)

    def rows(m, **over):
        ys = [Buf(n) for _ in range(m)]
        r = [dict(W, epi=STORE, x=T(x), y=y.t) for x, y in zip(xs_fp32(rng, m, k), ys)]
        for i, d in over.items():
            r[int(i[1:])].update(d)
        return r, ys

    def refused(r, ys, code):
        with pytest.raises(_lib.LlmiError, match=rf"\({code}\)"):
            ops.debug_gemv_rows(r)
        assert all(y.untouched() for y in ys), "a refused call wrote an output"

    refused(*rows(1), code=-1)                                  # m = 1
    refused(*rows(9), code=-1)                                  # m = 9
    refused(*rows(3, r2=dict(w=W_other["w"])), code=-1)         # another weight matrix
    refused(*rows(3, r1=dict(n_rows=n - 1)), code=-1)           # another shape
    refused(*rows(2, r1=dict(epi=ADD, resid=T(np.zeros(n, np.float32)))), code=-1)  # another epilogue
    g = gamma_args(rng, k, True)
    r, ys = rows(2)
    for d in r:                                                  # kpar is a single-row form
        d.update(g, kpar=2, x_fixed=T(np.zeros(k, np.int64)))
        d.pop("x")
    refused(r, ys, code=-2)
    r, ys = rows(2)
    for d in r:                                                  # fp32 x with RMSNorm: not a token-step form
        d.update(g)
    refused(r, ys, code=-2)


@pytest.mark.parametrize("wdt", ["f16", "i8", "f32"])
def test_linear_rows_equal_single_row_calls(ops, wdt):
    """llmi_linear with m = 2 .. 8 (routed to the multi-row GEMV) equals m calls with m = 1.
    A guard on the routing: it holds before the multi-row kernel exists too."""
    rng = np.random.default_rng(7)
    n, k = N_ROWS, K_TAIL[wdt]
    W = weights(wdt, n, k, seed=8)
    for m in range(2, 9):
        x = T(rng.standard_normal((m, k)).astype(np.float32))
        y = ops.launchLinearGemm(x, W["w"], W.get("scales"))
        for i in range(m):
            yi = ops.launchLinearGemm(x[i:i + 1], W["w"], W.get("scales"))
            assert torch.equal(y[i].view(torch.int32), yi[0].view(torch.int32)), (wdt, m, i)
