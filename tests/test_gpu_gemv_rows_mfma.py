"""The matrix-core multi-row GEMV (llmi_debug_gemv_rows_mfma, gemv_rows_mfma.hip) against float64,
one launch form at a time, at the project's GEMM / GEMV bar: the largest rel-L2 over the
activation rows below 2e-6. Bitwise: x_out and seed_dst, the sentinels past every buffer, and a
row's independence of m, of its column and of its neighbours.

Shapes: 37 weight rows (an odd tail tile), pair_off 19, k = 544 (17 MFMA steps: the 8 waves'
K slices are 3, 3, 3, 3, 3, 2, 0, 0 steps; int8: 34 chunks, a half-filled last load step), and
fp16 at k = 11008, m = 8 (43 steps a wave; three launches of the LDS-staged kernel). grid = 1
(ksplit: one workgroup a K slice) makes one workgroup stream every tile: the prefetch across
tiles, both LDS buffers and a rotating epilogue wave."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402

DEV, PAD, FX, BAR = "cuda", 64, 2.0 ** 32, 2e-6
N_ROWS, PO, K, SEED_N = 37, 19, 544, 300
STORE, ADD, SILU, ARGMAX, ATOMIC = range(5)
F32, I64 = torch.float32, torch.int64
_SENT = {F32: (torch.int32, 0x7FC0BEEF), I64: (I64, 0x5A5A5A5A5A5A5A5A)}
# form -> (shared fields, per-row inputs, per-row outputs: field -> (dtype, length))
FORMS = {
    "store": (dict(epi=STORE), ("x_fixed",), dict(y=(F32, "n_out"), x_out=(F32, "k"))),
    "silu": (dict(epi=SILU, pair_off=PO, seed_n=SEED_N, seed_keep=1), ("x_fixed", "seed_src"),
             dict(y=(F32, "n_out"), seed_dst=(I64, "seed_n"))),
    "atomic_single": (dict(epi=ATOMIC, yacc_single=1), ("x", "yacc_base"), dict(yacc=(I64, "n"), yacc_copy=(I64, "n"))),
    "atomic_ksplit": (dict(epi=ATOMIC), ("x",), dict(yacc=(I64, "n"))),
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buf:
    """n elements + PAD sentinels, the logical part NaN / garbage unless init is given."""

    def __init__(self, n, dtype=F32, init=None):
        it, self.pat = _SENT[dtype]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t, self.n = self.raw.view(dtype), n
        if init is not None:
            self.t[:n] = T(np.asarray(init))

    def get(self):  # the logical part's raw bits on the host, the sentinels checked
        torch.cuda.synchronize()
        assert bool((self.raw[self.n:] == self.pat).all()), "a store past the buffer's logical end"
        return self.raw[:self.n].cpu().numpy()


class Case:
    """One weight matrix and launch form, and 11 rows of inputs: x = (1 + i) N(0, 1) with planted
    +-300 and +-1e-6, a base and a seed."""

    def __init__(self, wdt, form, k=K, seed=0, grid=0, **over):
        rng = np.random.default_rng([seed, k, list(FORMS).index(form), int(wdt == "i8")])
        shared, self.ins, self.outs = FORMS[form]
        self.form, self.k, self.seed_n = form, k, SEED_N
        self.n = n = 2 * PO if form == "silu" else N_ROWS
        self.n_out = PO if form == "silu" else n
        if wdt == "i8":
            q = rng.integers(-127, 128, (n, k)).astype(np.int8)
            s = (0.002 + 0.001 * rng.random(n)).astype(np.float16)
            self.common = dict(w=T(q), scales=T(s), w_dtype=_lib.I8)
            self.w64 = q.astype(np.float64) * s.astype(np.float64)[:, None]
        else:
            w = (0.05 * rng.standard_normal((n, k))).astype(np.float16)
            self.common = dict(w=T(w), w_dtype=_lib.F16)
            self.w64 = w.astype(np.float64)
        self.gamma = None
        if "x_fixed" in self.ins:  # fp16 gamma for the store form, fp32 for silu
            g = (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16 if form == "store" else np.float32)
            self.gamma = g.astype(np.float64)
            self.common.update(gamma=T(g), g_dtype=_lib.F16 if form == "store" else _lib.F32, eps=1e-5)
        self.common.update(shared, n_rows=n, k=k, grid=grid, **(dict(ksplit=k // 32) if form == "atomic_ksplit" else {}))
        self.common.update(over)
        self.rows = []
        for i in range(11):
            x = (1.0 + i) * rng.standard_normal(k)
            x[rng.choice(k, 8, replace=False)] = [300, -300, 1e-6, -1e-6, 300, -1e-6, 1e-6, -300]
            r = dict(yacc_base=rng.integers(-2 ** 40, 2 ** 40, n), seed_src=rng.integers(-2 ** 50, 2 ** 50, SEED_N),
                     x=x.astype(np.float32))
            if self.gamma is not None:
                r["x_fixed"] = np.rint(x * FX).astype(np.int64)
                r["x"] = r["x_fixed"].astype(np.float32) * np.float32(1.0 / FX)  # from_fixed: one rounding
            self.rows.append(r)

    def ref(self, i):
        x = self.rows[i]["x"].astype(np.float64)
        if self.gamma is None:
            return self.w64 @ x
        y = self.w64 @ (x * self.gamma) / np.sqrt(np.mean(x * x) + 1e-5)
        return y if self.form == "store" else y[:PO] / (1.0 + np.exp(-y[:PO])) * y[PO:]

    def launch(self, ops, idx):
        """One launch over the rows idx (in that order): per row a dict of host outputs."""
        bufs = [{f: Buf(getattr(self, ln), dt, self.rows[i]["yacc_base"] if self.form == "atomic_ksplit" else None)
                 for f, (dt, ln) in self.outs.items()} for i in idx]
        ops.debug_gemv_rows_mfma([dict(self.common, **{f: T(self.rows[i][f]) for f in self.ins},
                                       **{f: bb.t for f, bb in b.items()}) for i, b in zip(idx, bufs)])
        return [{f: bb.get() for f, bb in b.items()} for b in bufs]


def check(case, ops, m):
    worst = 0.0
    for i, out in enumerate(case.launch(ops, range(m))):
        ref, r = case.ref(i), case.rows[i]
        got = out["y"].view(np.float32) if "y" in out else (out["yacc"] - r["yacc_base"]) / FX  # (yacc - base) * 2^-32
        worst = max(worst, np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
        if "x_out" in out:
            assert np.array_equal(out["x_out"], r["x"].view(np.int32)), "x_out is not the fp32 image of x_fixed"
        if "seed_dst" in out:
            assert np.array_equal(out["seed_dst"], r["seed_src"]), "seed_dst is not a copy of seed_src"
        if "yacc_copy" in out:
            assert np.array_equal(out["yacc_copy"], out["yacc"])
    print(f"rel-L2 {case.form} k={case.k} m={m}: {worst:.3e}")
    assert worst < BAR, worst


@pytest.mark.parametrize("m,one_wg", [(1, False), (3, False), (8, False), (8, True)])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wdt", ["f16", "i8"])
def test_against_float64(ops, wdt, form, m, one_wg):
    check(Case(wdt, form, grid=(K // 32 if form == "atomic_ksplit" else 1) if one_wg else 0), ops, m)


def test_against_float64_k11008(ops):
    """The 7B down projection's k, 8 rows, ONE launch (single producer, as down_args gives it)."""
    check(Case("f16", "atomic_single", k=11008), ops, 8)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wdt", ["f16", "i8"])
def test_row_independent_of_m_column_and_neighbours(ops, wdt, form):
    case = Case(wdt, form, seed=1)
    full = case.launch(ops, range(8))
    # rows 0 and 5 alone (m = 1, column 0); rows 6 and 2 in other columns among other neighbours
    for idx in ([0], [5], [9, 6, 10, 2]):
        for got, i in zip(case.launch(ops, idx), idx):
            for f in full[i] if i < 8 else ():
                assert np.array_equal(got[f], full[i][f]), f"row {i}: {f} depends on m, its column or its neighbours"


@pytest.mark.parametrize("what", ["argmax", "f32_weights", "k536", "kpar"])
def test_refusals_launch_nothing(ops, what):
    over = dict(argmax=dict(epi=ARGMAX, partials=T(np.zeros(64, np.int64))), k536={}, kpar=dict(kpar=2),
                f32_weights=dict(w=T(np.ones((N_ROWS, K), np.float32)), w_dtype=_lib.F32))[what]
    case = Case("f16", "store", k=536 if what == "k536" else K, **over)
    bufs = [Buf(N_ROWS), Buf(N_ROWS)]
    with pytest.raises(_lib.LlmiError, match=r"\(-2\).*gemv_rows_mfma: "):
        ops.debug_gemv_rows_mfma([dict(case.common, x_fixed=T(case.rows[i]["x_fixed"]), y=y.t) for i, y in enumerate(bufs)])
    assert all(bool((y.raw == y.pat).all()) for y in bufs), "a refused call wrote an output"
