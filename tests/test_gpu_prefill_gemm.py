"""Operator-level tests of the prefill GEMMs (gemm2.hip, gemm3.hip), one launch form at a time
through the test hook llmi_debug_gemm: the planes are fed directly, so the operation under test
is exactly sum_p A_p W^T (op)= into y, a slab slice or the gate_up product. Every case asserts,
through llmi_debug_gemm_plan, the form it names (row tile, workgroups, stream-K slots).

Sections and bars, and where each bar comes from:
  A  integer planes (a_hi, a_lo in [-4, 4], W and W8 in [-3, 3], drawn independently): every
     product and partial sum is exact in fp32 (|sum| <= 4 x 3 x 2 x 1024 < 2^24) whatever the
     order, so y is BITWISE the exact matmul (float64 BLAS on these integers is exact: it is
     the int64 product) for store, y0 + matmul for add, and for slab every slice is the matmul
     over exactly its K range (gemm2: [s K / S, (s + 1) K / S); gemm3: K tiles [s KT / S,
     (s + 1) KT / S) of each plane, 128-deep tiles under lo8). lo8: a_lo is e4m3 bytes of
     integers, W8 an independent integer matrix in e4m3 and w8_exp = -12, so the two E8M0 scales
     cancel: the block-scaled MFMA adds these integers exactly too (measured: every lo8 case
     bitwise), so lo8 is held to the same bitwise bar.
  B  real data (x normal, hi = fp16(x), lo = fp16(x - hi); W fp16 N(0, 1/k)) against float64 of
     the same planes: the MAXIMUM OVER ROWS of the row's rel-L2 < 2e-6, the project's GEMM bar.
     lo8 planes come from llmi_debug_rows_split and W8 from llmi_debug_w8_prepare; the reference
     decodes the bytes with torch.float8_e4m3fn on the CPU. One lo8 case also compares with
     float64 x W^T of the unsplit x: <= 2 x the error of the numpy model of the planes, which is
     computed here and printed (the factor covers the fp32 accumulation the model does not round).
  C  gate_up: integer planes, W scaled by a power of two, gate and up rows from different
     distributions; a few rows scaled up so that gate passes -89, where expf overflows and the
     product is -0 x up. fp32 y per-row rel-L2 < 2e-6 against float64 silu(g) u of the exact g, u;
     the numpy fp32 restatement g / (1 + exp(-g)) u is held to the same bar on the same inputs,
     so the bar is not taken from the kernel. Planes bitwise fp16(v), fp16(v - hi) of the fp32
     output v of the same kernel; the e4m3 lo bytes as decoded values against
     f8_round((v - hi) 4096), v from a one-plane launch over [hi | lo] x [W | W8] that has the
     same exact accumulators.
  D  stream-K: bitwise the plain launch (and the matmul) on integer data, two launches in a row
     bitwise equal, no error bit, and a captured launch replayed three times.
  E  llmi_linear's gemm2 launch bitwise the hook's; every refusal of the launchers through both
     hooks with every output untouched; two identical launches bitwise.
Every output carries 64 sentinels behind its end, ldy = n + 8, two more rows than m, and starts
as NaNs: get() checks the sentinels, read() that the padding columns and the rows >= m are
untouched. A planes have lda = k + 8 with NaN padding, the fp8 rows NaN bytes behind their k.

Found by section C in gemm3's plane epilogue and fixed there ("Prefill GEMMs, one form
at a time"): an exact -0 product came out as +0 in y_hi (the multiply was folded into the
conversion with a +0 addend), and the e4m3 lo bytes were converted from the fp16 lo instead of the
fp32 remainder (rounded twice: 555 of 115200 bytes one e4m3 step off at (300, 384, 256)).
Measured on an MI355X: A and D bitwise; B max row 2.9e-7 (gemm2), 2.1e-7 (gemm3; lo8 2.1e-7), the
lo8 kernel 7.367e-6 against the unsplit product with the planes' model at 7.365e-6 (the hi plane
alone: 2.1e-4); C fp32 y max row 4.7e-8, the numpy restatement's own figure.

Not covered (not reachable from any caller, not exposed by the hook): w_kblock != 0 (head-major
W blocks) and gemm3_silu_bal_kernel (bal_slab is never set). gemm.hip, the first-generation GEMM
of the int8 engines, has its own file: tests/test_gpu_gemm1.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402

DEV = "cuda"
BAR = 2e-6
PAD = 64
STORE, ADD, SILU, SLAB = 0, 1, 2, 5
NAN8 = 0x7F  # an e4m3 NaN


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def row_err(out, ref):
    """max over rows of the row's rel-L2."""
    o = np.asarray(out, np.float64).reshape(-1, out.shape[-1])
    r = np.asarray(ref, np.float64).reshape(-1, out.shape[-1])
    return float((np.linalg.norm(o - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-30)).max())


def report(group, what, r):
    print(f"[rel-L2] {group}: {what}: {r:.3e}")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_SENT = {torch.float32: (torch.int32, 0x7FC0BEEF),   # NaNs
         torch.float16: (torch.int16, 0x7EEF),
         torch.uint8: (torch.uint8, 0xA5)}


class Buf:
    """n elements + PAD sentinels. The logical part starts as `init` or as the sentinel pattern
    (a NaN for the float types); get() checks the sentinels."""

    def __init__(self, n, dtype=torch.float32, init=None):
        it, self.pat = _SENT[dtype]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t = self.raw.view(dtype)
        self.n = n
        if init is not None:
            self.t[:n] = T(np.asarray(init).reshape(-1))

    def get(self):
        torch.cuda.synchronize()
        assert (self.raw[self.n:].cpu().numpy() == self.pat).all(), "a store past the buffer's logical end"
        return self.t[:self.n].cpu().numpy().copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


class Out:
    """[rows, ld] elements in a Buf whose logical part is [m, n] (starting as y0 or the pattern);
    read() returns it and checks that every other element still holds the pattern."""

    def __init__(self, rows, ld, m, n, dtype=torch.float32, y0=None):
        self.b = Buf(rows * ld, dtype)
        self.rows, self.ld, self.m, self.n = rows, ld, m, n
        self.t = self.b.t
        if y0 is not None:
            self.t[:rows * ld].view(rows, ld)[:m, :n] = T(y0)

    def read(self):
        a = self.b.get().reshape(self.rows, self.ld)
        u = bits(a)
        pat = u.dtype.type(self.b.pat)
        assert (u[self.m:] == pat).all(), "a store to a row >= m"
        assert (u[:self.m, self.n:] == pat).all(), "a store to a padding column"
        return a[:self.m, :self.n].copy()

    def refill(self):
        self.b.raw.fill_(self.b.pat)


def f8_decode(b):
    return torch.from_numpy(np.ascontiguousarray(b, np.uint8)).view(torch.float8_e4m3fn).float().numpy()


def f8_encode(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def f8_round(x):
    """decoded torch.float8_e4m3fn (CPU) of clamp(x, +-448)."""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return torch.clamp(x, -448.0, 448.0).to(torch.float8_e4m3fn).float().numpy()


def mm(a, w):
    """a w^T in float64: exact (the int64 product) on the integer inputs."""
    return np.asarray(a, np.float64) @ np.asarray(w, np.float64).T


def plan_model(kernel, m, n, k, epi, ks):
    """The launchers' rule restated (as tests/test_lib_cpu.py): (bm, workgroups, 0)."""
    s = ks if epi == SLAB else 1
    if kernel == 2:
        nt = (n // 2) // 64 if epi == SILU else n // 128
        bm = 128 if epi == SLAB or -(-m // 128) * nt >= 256 else 64
    else:
        nt = (n // 2) // 128 if epi == SILU else n // 256
        bm = 256
    return bm, -(-m // bm) * nt * s, 0


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ one launch
class Run:
    pass


def padded(a, ld, fill):
    """[m, k] -> [m, ld] with `fill` behind the k used columns."""
    out = np.full((a.shape[0], ld), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def run(ops, kernel, m, n, k, hi, w, lo=None, lo8=None, w8=None, w8_exp=0, epi=STORE, ks=0, y0=None, fmt="f32",
        stream_k=0, pmax=None, lda=None, launches=1):
    """One llmi_debug_gemm launch on fresh device copies. hi / lo: fp16 [m, k]; lo8: e4m3 bytes
    [m, k] (with w8 bytes [n, k]) instead of lo. fmt (gate_up): "f32", "hi", "planes" or "lo8".
    pmax: the stream-K slots the plan must report (None: the plain form, restated in plan_model).
    Returns the read-back logical outputs, padding and sentinels checked."""
    lda = lda or k + 8
    planes = 1 if lo is None and lo8 is None else 2
    n_out = n // 2 if epi == SILU else n
    ldy = n_out + 8
    keep = [T(padded(hi.astype(np.float16), lda, np.float16(np.nan))), T(w.astype(np.float16))]
    a = dict(kernel=kernel, a_hi=keep[0], planes=planes, lda=lda, w=keep[1], m=m, n=n, k=k, epi=epi, ldy=ldy,
             ksplit=ks, stream_k=stream_k)
    if lo is not None:
        keep.append(T(padded(lo.astype(np.float16), lda, np.float16(np.nan))))
        a["a_lo"] = keep[-1]
    if lo8 is not None:
        keep.append(T(padded(lo8, 2 * lda, np.uint8(NAN8))))
        keep.append(T(padded(w8, 2 * k, np.uint8(NAN8))))
        a.update(a_lo=keep[-2], lo8=1, w8=keep[-1], w8_exp=w8_exp)
    o = {}
    if epi == SLAB:
        o["slab"] = Out(ks * m + 2, ldy, ks * m, n)
        o["y"] = Out(2, ldy, 0, 0)                     # gemm2 wants it non-null; never written
    elif epi != SILU or fmt == "f32":
        o["y"] = Out(m + 2, ldy, m, n_out, y0=y0)
    else:
        o["y_hi"] = Out(m + 2, ldy, m, n_out, torch.float16)
        if fmt == "planes":
            o["y_lo"] = Out(m + 2, ldy, m, n_out, torch.float16)
        elif fmt == "lo8":
            o["y_lo"] = Out(m + 2, 2 * ldy, m, n_out, torch.uint8)
    a.update({key: v.t for key, v in o.items()})
    r = Run()
    r.plan = ops.debug_gemm_plan(**a)
    if pmax is None:
        assert r.plan == plan_model(kernel, m, n, k, epi, ks), (r.plan, kernel, m, n, k, epi, ks)
    else:
        assert 1 <= r.plan[2] <= 3, f"stream-K was not taken: plan {r.plan}"
        assert r.plan == (256, n_cu(), pmax), r.plan
    r.reads = []
    for i in range(launches):
        if i:
            for v in o.values():
                v.refill()
            if y0 is not None:
                o["y"].t[:(m + 2) * ldy].view(m + 2, ldy)[:m, :n_out] = T(y0)
        ops.debug_gemm(**a)
        r.reads.append({key: v.read() for key, v in o.items()})
    for key, v in r.reads[0].items():
        setattr(r, key, v)
    if epi == SLAB:
        r.slab = r.slab.reshape(ks, m, n)
    return r


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ne = bits(a) != bits(b)
    if ne.any():
        i = tuple(int(x) for x in np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} elements differ, first at {i}: {a[i]!r} != {b[i]!r}; "
                             f"rows {sorted(set(np.argwhere(ne)[:, -2].tolist()))[:8]}")


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def int_case(m, n, k):
    """Integer planes and weights, drawn independently (non-symmetric, every row and column its own)."""
    rng = np.random.default_rng([11, m, n, k])
    c = Run()
    c.hi = rng.integers(-4, 5, (m, k)).astype(np.float32)
    c.lo = rng.integers(-4, 5, (m, k)).astype(np.float32)
    c.w = rng.integers(-3, 4, (n, k)).astype(np.float32)
    c.w8 = rng.integers(-3, 4, (n, k)).astype(np.float32)
    c.y0 = rng.integers(-1000, 1001, (m, n)).astype(np.float32)
    return c


def int_run(ops, kernel, m, n, k, form, **kw):
    """form: 1 / 2 planes or "lo8"; returns (run, the exact planes-times-weights pairs)."""
    c = int_case(m, n, k)
    if form == "lo8":
        r = run(ops, kernel, m, n, k, c.hi, c.w, lo8=f8_encode(c.lo), w8=f8_encode(c.w8), w8_exp=-12, **kw)
        return r, [(c.hi, c.w), (c.lo, c.w8)]
    r = run(ops, kernel, m, n, k, c.hi, c.w, lo=c.lo if form == 2 else None, **kw)
    return r, [(c.hi, c.w)] + ([(c.lo, c.w)] if form == 2 else [])


def slab_ref(kernel, pairs, k, ks, lo8):
    """[ks, m, n]: every slice's exact sum over its K range."""
    out = []
    for s in range(ks):
        if kernel == 2:
            k0, k1 = s * (k // ks), (s + 1) * (k // ks)
        else:
            unit = 128 if lo8 else 64
            kt = k // unit
            k0, k1 = (s * kt // ks) * unit, ((s + 1) * kt // ks) * unit
        out.append(sum(mm(a[:, k0:k1], w[:, k0:k1]) for a, w in pairs))
    return np.stack(out)


# ------------------------------------------------------------------ A. integer-exact, bitwise
G2_STORE = [(1, 128, 64), (63, 128, 128), (64, 256, 192), (65, 128, 256), (129, 384, 320), (300, 128, 576),
            (257, 11008, 192), (300, 11008, 64)]


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("m,n,k", G2_STORE)
def test_a_gemm2_store(ops, m, n, k, planes):
    """KT = 1, 2, 3, 4, 5, 9 against the 3 stages; the last two shapes take 128-row tiles by
    their tile count (asserted through the plan)."""
    r, pairs = int_run(ops, 2, m, n, k, planes)
    assert r.plan[0] == (128 if n == 11008 else 64)
    same_bits(r.y, sum(mm(a, w) for a, w in pairs).astype(np.float32), "y")


@pytest.mark.parametrize("m,n,k,planes", [(77, 256, 192, 2), (130, 128, 64, 1)])
def test_a_gemm2_add(ops, m, n, k, planes):
    c = int_case(m, n, k)
    r, pairs = int_run(ops, 2, m, n, k, planes, epi=ADD, y0=c.y0)
    same_bits(r.y, (c.y0 + sum(mm(a, w) for a, w in pairs)).astype(np.float32), "y0 + a w^T")


@pytest.mark.parametrize("m,n,k,ks", [(16, 128, 64, 1), (100, 256, 512, 2), (130, 128, 192, 3), (64, 128, 512, 8)])
def test_a_gemm2_slab(ops, m, n, k, ks):
    for planes in (1, 2):
        r, pairs = int_run(ops, 2, m, n, k, planes, epi=SLAB, ks=ks)
        assert r.plan[0] == 128
        same_bits(r.slab, slab_ref(2, pairs, k, ks, False).astype(np.float32), f"slab, {planes} plane(s)")


G3_ONE = [(1, 256, 128), (255, 256, 192), (256, 512, 256), (257, 256, 320), (257, 256, 384), (300, 512, 448),
          (513, 256, 128), (513, 256, 192), (1, 256, 448)]
G3_TWO = [(300, 256, 128), (257, 512, 192), (255, 256, 256), (300, 256, 320)]
G3_LO8 = [(300, 256, 128), (1, 256, 256), (257, 512, 384), (256, 256, 512), (300, 256, 640)]


@pytest.mark.parametrize("m,n,k,form", [s + (1,) for s in G3_ONE] + [s + (2,) for s in G3_TWO] +
                         [s + ("lo8",) for s in G3_LO8])
def test_a_gemm3_store(ops, m, n, k, form):
    """One plane: KT = 2 .. 7 (KT 2, KT 3, even and odd, the paired-steady / steady / generic tile
    bodies); two planes: 4 .. 10 virtual tiles; lo8: 3, 6, 9, 12, 15 virtual tiles with the fp8
    pass starting after 2, 4, 6, 8, 10 fp16 tiles."""
    r, pairs = int_run(ops, 3, m, n, k, form)
    same_bits(r.y, sum(mm(a, w) for a, w in pairs).astype(np.float32), "y")


@pytest.mark.parametrize("m,n,k,form", [(300, 256, 128, 2), (257, 512, 192, 1)])
def test_a_gemm3_add(ops, m, n, k, form):
    c = int_case(m, n, k)
    r, pairs = int_run(ops, 3, m, n, k, form, epi=ADD, y0=c.y0)
    same_bits(r.y, (c.y0 + sum(mm(a, w) for a, w in pairs)).astype(np.float32), "y0 + a w^T")


@pytest.mark.parametrize("m,n,k,ks,form", [(300, 256, 320, 2, 1), (300, 256, 320, 2, 2), (300, 512, 832, 4, 2),
                                           (300, 256, 384, 2, "lo8"), (300, 512, 1152, 8, "lo8")])
def test_a_gemm3_slab(ops, m, n, k, ks, form):
    """Uneven slices: 2 + 3 tiles; 3, 3, 3, 4; lo8 with 1 + 2 fp8 tiles; lo8 with seven slices of
    one fp8 tile and one of two (the small twin of the engine's down GEMM)."""
    r, pairs = int_run(ops, 3, m, n, k, form, epi=SLAB, ks=ks)
    same_bits(r.slab, slab_ref(3, pairs, k, ks, form == "lo8").astype(np.float32), "slab")


# ------------------------------------------------------------------ B. real data against float64
@functools.lru_cache(maxsize=None)
def real_case(m, n, k):
    rng = np.random.default_rng([12, m, n, k])
    c = Run()
    c.x = rng.standard_normal((m, k)).astype(np.float32)
    c.hi = c.x.astype(np.float16)
    c.lo = (c.x - c.hi.astype(np.float32)).astype(np.float16)
    c.w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float16)
    c.y0 = rng.standard_normal((m, n)).astype(np.float32)
    return c


def lo8_planes(ops, c, m, n, k):
    """The production producers' planes and weight copy for c: hi fp16 [m, k], lo e4m3 bytes
    [m, k], w8 bytes [n, k] and its exponent."""
    lda = k + 8
    x = T(c.x)
    hi = torch.zeros(m, lda, dtype=torch.float16, device=DEV)
    lo = torch.full((m, 2 * lda), NAN8, dtype=torch.uint8, device=DEV)
    ops.debug_rows_split(x, m, k, hi=hi, lo=lo.view(torch.float16), ldh=lda, lo8=True)
    w8 = torch.full((n, 2 * k), NAN8, dtype=torch.uint8, device=DEV)
    e = ops.debug_w8_prepare(T(c.w), w8)
    torch.cuda.synchronize()
    return hi.cpu().numpy()[:, :k], lo.cpu().numpy()[:, :k], w8.cpu().numpy()[:, :k], e


def real_run(ops, kernel, m, n, k, form, epi, ks=0, launches=1):
    """One section-B launch and its float64 reference of the same planes ([ks, m, n] for slab)."""
    c = real_case(m, n, k)
    kw = dict(epi=epi, ks=ks, y0=c.y0 if epi == ADD else None, launches=launches)
    if form == "lo8":
        hi, lo8, w8, e = lo8_planes(ops, c, m, n, k)
        same_bits(hi, c.hi, "rows_split hi")
        r = run(ops, kernel, m, n, k, hi, c.w, lo8=lo8, w8=w8, w8_exp=e, **kw)
        pairs = [(hi, c.w), (f8_decode(lo8).astype(np.float64) / 4096.0, f8_decode(w8).astype(np.float64) * 2.0 ** -e)]
    else:
        r = run(ops, kernel, m, n, k, c.hi, c.w, lo=c.lo if form == 2 else None, **kw)
        pairs = [(c.hi, c.w)] + ([(c.lo, c.w)] if form == 2 else [])
    if epi == SLAB:
        return r, slab_ref(kernel, pairs, k, ks, form == "lo8"), c
    return r, sum(mm(a, w) for a, w in pairs) + (c.y0.astype(np.float64) if epi == ADD else 0.0), c


B_CASES = [(2, 129, 384, 320, 1, STORE, 0), (2, 300, 128, 576, 2, STORE, 0),
           (2, 130, 128, 64, 1, ADD, 0), (2, 77, 256, 192, 2, ADD, 0),
           (2, 130, 128, 192, 1, SLAB, 3), (2, 100, 256, 512, 2, SLAB, 2),
           (3, 257, 256, 320, 1, STORE, 0), (3, 257, 512, 192, 2, STORE, 0), (3, 257, 512, 384, "lo8", STORE, 0),
           (3, 257, 512, 192, 1, ADD, 0), (3, 300, 256, 128, 2, ADD, 0), (3, 300, 256, 640, "lo8", ADD, 0),
           (3, 300, 256, 320, 1, SLAB, 2), (3, 300, 512, 832, 2, SLAB, 4), (3, 300, 512, 1024, "lo8", SLAB, 8)]


@pytest.mark.parametrize("kernel,m,n,k,form,epi,ks", B_CASES)
def test_b_real_against_float64(ops, kernel, m, n, k, form, epi, ks):
    r, ref, _ = real_run(ops, kernel, m, n, k, form, epi, ks)
    e = row_err(r.slab if epi == SLAB else r.y, ref)
    report("B", f"gemm{kernel} {form} epi {epi} ({m}, {n}, {k}) ks {ks} max row", e)
    assert e < BAR


def test_b_lo8_against_the_unsplit_product(ops):
    """The fp8 lo plane's "~2^-15 per product": the kernel against float64 x W^T of the fp32 x,
    within 2 x the error of the numpy model of its planes against that product."""
    m, n, k = 257, 512, 384
    r, model, c = real_run(ops, 3, m, n, k, "lo8", STORE)
    full = mm(c.x, c.w)
    em, ek = rel(model, full), rel(r.y, full)
    report("B", "lo8 planes model against the unsplit x W^T", em)
    report("B", "lo8 kernel against the unsplit x W^T", ek)
    report("B", "fp16 hi plane alone against the unsplit x W^T", rel(mm(c.hi, c.w), full))
    assert ek <= 2 * em


# ------------------------------------------------------------------ C. the gate_up epilogue
@functools.lru_cache(maxsize=None)
def silu_case(m, inter, k):
    """Integer planes, gate rows in [-3, 3] / 4 and up rows in [0, 3] / 32 (another distribution:
    a swapped or shifted pairing is off by orders of magnitude); rows 0, m / 2 and m - 1 are
    scaled by 4 so that gate passes +-100."""
    rng = np.random.default_rng([13, m, inter, k])
    c = Run()
    c.hi = rng.integers(-4, 5, (m, k)).astype(np.float32)
    c.lo = rng.integers(-4, 5, (m, k)).astype(np.float32)
    for row in {0, m // 2, m - 1}:
        c.hi[row] *= 4
        c.lo[row] *= 4
    c.wg = rng.integers(-3, 4, (inter, k)).astype(np.float32) / 4
    c.wu = rng.integers(0, 4, (inter, k)).astype(np.float32) / 32
    c.w = np.concatenate([c.wg, c.wu])
    c.g = mm(c.hi + c.lo, c.wg)   # exact: multiples of 1/4 (1/32) far below 2^24 of them
    c.u = mm(c.hi + c.lo, c.wu)
    with np.errstate(over="ignore"):
        c.ref = c.g / (1.0 + np.exp(-c.g)) * c.u
        g32, u32 = c.g.astype(np.float32), c.u.astype(np.float32)
        c.np32 = g32 / (np.float32(1) + np.exp(-g32)) * u32
    return c


C_SHAPES = [(2, 65, 64, 128), (2, 130, 192, 64), (2, 257, 5504, 64), (3, 1, 128, 128), (3, 257, 256, 192)]


@pytest.mark.parametrize("kernel,m,inter,k", C_SHAPES)
def test_c_gate_up(ops, kernel, m, inter, k):
    """fp32 y (gemm3: direct stores), then y_hi alone and y_hi + y_lo (gemm3: through LDS),
    bitwise the planes of that y."""
    c = silu_case(m, inter, k)
    assert (c.g < -100).any() and (c.g > 100).any() and np.abs(c.g).max() < 2000
    e32 = row_err(c.np32, c.ref)
    report("C", f"numpy fp32 restatement ({m}, {inter}, {k}) max row", e32)
    assert e32 < BAR
    r = run(ops, kernel, m, 2 * inter, k, c.hi, c.w, lo=c.lo, epi=SILU)
    assert r.plan[0] == {2: 128 if inter == 5504 else 64, 3: 256}[kernel]
    e = row_err(r.y, c.ref)
    report("C", f"gemm{kernel} gate_up fp32 y ({m}, {inter}, {k}) max row", e)
    assert e < BAR
    v = r.y
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    r1 = run(ops, kernel, m, 2 * inter, k, c.hi, c.w, lo=c.lo, epi=SILU, fmt="hi")
    same_bits(r1.y_hi, hi, "y_hi alone")
    r2 = run(ops, kernel, m, 2 * inter, k, c.hi, c.w, lo=c.lo, epi=SILU, fmt="planes")
    same_bits(r2.y_hi, hi, "y_hi")
    same_bits(r2.y_lo, lo, "y_lo")
    # one plane: the same epilogue on other accumulators
    r3 = run(ops, kernel, m, 2 * inter, k, c.hi + c.lo, c.w, epi=SILU)
    same_bits(r3.y, v, "one plane of hi + lo")


def test_c_gate_up_lo8(ops):
    """gemm3 with the fp8 lo plane in and out. W8 holds the integers of W (w8_exp -10 puts its
    products on W's 1/4 grid), so a one-plane launch over [hi | lo] x [W | W8 / 4] has the same
    exact accumulators and gives v."""
    m, inter, k = 300, 384, 256
    c = silu_case(m, inter, k)
    rng = np.random.default_rng([14, m, inter, k])
    w8 = np.concatenate([rng.integers(-3, 4, (inter, k)), rng.integers(0, 4, (inter, k))]).astype(np.float32)
    lo = np.clip(c.lo, -16, 16)
    cat_a, cat_w = np.concatenate([c.hi, lo], axis=1), np.concatenate([c.w, w8 / 4], axis=1)
    rv = run(ops, 3, m, 2 * inter, 2 * k, cat_a, cat_w, epi=SILU)
    g, u = mm(cat_a, cat_w[:inter]), mm(cat_a, cat_w[inter:])
    with np.errstate(over="ignore"):
        e = row_err(rv.y, g / (1.0 + np.exp(-g)) * u)
    report("C", f"gemm3 gate_up fp32 y, one plane of [hi | lo] ({m}, {inter}, {2 * k}) max row", e)
    assert e < BAR
    v = rv.y
    hi = v.astype(np.float16)
    r = run(ops, 3, m, 2 * inter, k, c.hi, c.w, lo8=f8_encode(lo), w8=f8_encode(w8), w8_exp=-10, epi=SILU, fmt="lo8")
    same_bits(r.y_hi, hi, "y_hi")
    want = f8_round((v - hi.astype(np.float32)) * np.float32(4096.0))
    got = f8_decode(r.y_lo)
    assert np.array_equal(got, want), f"{int((got != want).sum())} lo bytes differ"


# ------------------------------------------------------------------ D. stream-K
SK_CASES = [(SILU, 2, 300, 2 * 4096, 512, 3), (SILU, 2, 300, 2 * 8192, 256, 1), (SILU, "lo8", 512, 2 * 6144, 512, 2),
            (STORE, 2, 300, 8192, 512, 3), (STORE, "lo8", 300, 12288, 512, 2)]


def sk_run(ops, epi, form, m, n, k, **kw):
    if epi == STORE:
        return int_run(ops, 3, m, n, k, form, **kw)
    c = silu_case(m, n // 2, k)
    if form == "lo8":
        rng = np.random.default_rng([15, m, n, k])
        w8 = np.concatenate([rng.integers(-3, 4, (n // 2, k)), rng.integers(0, 4, (n // 2, k))]).astype(np.float32)
        return run(ops, 3, m, n, k, c.hi, c.w, lo8=f8_encode(np.clip(c.lo, -16, 16)), w8=f8_encode(w8), w8_exp=-10,
                   epi=SILU, fmt="lo8", **kw), None
    return run(ops, 3, m, n, k, c.hi, c.w, lo=c.lo, epi=SILU, fmt="planes", **kw), None


@pytest.mark.parametrize("epi,form,m,n,k,pmax", SK_CASES)
def test_d_stream_k(ops, epi, form, m, n, k, pmax):
    """Each stream-K form (the plan must report the slots; a case that did not take stream-K
    fails): bitwise the plain launch (store: and the exact matmul), twice in a row, no error bit."""
    ops.stream_errors()
    r, pairs = sk_run(ops, epi, form, m, n, k, stream_k=1, pmax=pmax, launches=2)
    assert ops.stream_errors() == 0
    p, _ = sk_run(ops, epi, form, m, n, k)
    for key in r.reads[0]:
        same_bits(r.reads[0][key], p.reads[0][key], f"{key}: stream-K against the plain launch")
        same_bits(r.reads[1][key], r.reads[0][key], f"{key}: the second launch")
    if epi == STORE:
        same_bits(r.y, sum(mm(a, w) for a, w in pairs).astype(np.float32), "y")


def test_d_one_plane_declines(ops):
    """One fp16 plane without lo8: the plan reports no slots, and the launch is the plain one."""
    m, n, k = 300, 8192, 512
    r, pairs = int_run(ops, 3, m, n, k, 1, stream_k=1)     # run() asserts the plain plan
    assert r.plan[2] == 0
    same_bits(r.y, mm(*pairs[0]).astype(np.float32), "y")


def test_d_graph_replay(ops):
    """A captured stream-K launch replayed three times on its stream: every replay gets a fresh
    epoch (the kernel advances it), so each is bitwise the eager result with no error bit."""
    m, n, k = 300, 8192, 512
    c = int_case(m, n, k)
    want = (mm(c.hi, c.w) + mm(c.lo, c.w)).astype(np.float32)
    ldy = n + 8
    hi, lo, w = T(c.hi.astype(np.float16)), T(c.lo.astype(np.float16)), T(c.w.astype(np.float16))
    y = Out(m + 2, ldy, m, n)
    a = dict(kernel=3, a_hi=hi, a_lo=lo, planes=2, lda=k, w=w, m=m, n=n, k=k, epi=STORE, y=y.t, ldy=ldy, stream_k=1)
    assert ops.debug_gemm_plan(**a) == (256, n_cu(), 3)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ops.debug_gemm(**a)                      # eager: the stream's workspace and error word exist
        same_bits(y.read(), want, "eager")
        assert ops.stream_errors() == 0
        graph = torch.cuda.CUDAGraph()
        y.refill()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.debug_gemm(**a)
        for i in range(3):
            y.refill()
            graph.replay()
            same_bits(y.read(), want, f"replay {i}")
            assert ops.stream_errors() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ E. production, refusals, repeatability
def test_e_llmi_linear_launches_what_the_hook_launches(ops):
    """llmi_linear at (130, 10240, 64): gemm2 (m < 256) with ks = 1 because its 2 x 80 tiles of
    128 x 128 are >= 160, so y is the store epilogue's own output: bitwise the hook's launch on
    numpy-made planes of the same x."""
    m, n, k = 130, 10240, 64
    assert m < 256 and -(-m // 128) * (n // 128) >= 160
    c = real_case(m, n, k)
    y = ops.launchLinearGemm(T(c.x), T(c.w))
    torch.cuda.synchronize()
    r = run(ops, 2, m, n, k, c.hi, c.w, lo=c.lo, lda=k)
    same_bits(r.y, y.cpu().numpy(), "llmi_linear against the hook")
    e = row_err(r.y, mm(c.hi, c.w) + mm(c.lo, c.w))
    report("E", f"gemm2 store ({m}, {n}, {k}) max row", e)
    assert e < BAR


def test_e_refusals(ops):
    """Every LLMI_REQUIRE of gemm2_launch / gemm3_launch (and the hook's own), through both
    hooks: LlmiError, and no output buffer is touched."""
    m, n, k, lda, ldy = 64, 256, 256, 264, 264
    hi = torch.zeros(m, lda, dtype=torch.float16, device=DEV)
    lo = torch.zeros(m, 2 * lda, dtype=torch.float16, device=DEV)   # wide enough for the fp8 rows
    w = torch.zeros(n, k, dtype=torch.float16, device=DEV)
    w8 = torch.zeros(n, 2 * k, dtype=torch.uint8, device=DEV)
    outs = dict(y=Out(m, ldy, 0, 0), slab=Out(8 * m, ldy, 0, 0), y_hi=Out(m, ldy, 0, 0, torch.float16),
                y_lo=Out(m, 2 * ldy, 0, 0, torch.float16))
    P = {key: v.t.data_ptr() for key, v in outs.items()}
    base = dict(a_hi=hi, a_lo=lo, planes=2, lda=lda, w=w, m=m, n=n, k=k, epi=STORE, y=P["y"], ldy=ldy)
    l8 = dict(lo8=1, w8=w8, w8_exp=0)
    silu = dict(epi=SILU, y=None, y_hi=P["y_hi"], y_lo=P["y_lo"])
    slab = dict(epi=SLAB, slab=P["slab"], ksplit=2)
    both = [dict(a_hi=None), dict(w=None), dict(m=0), dict(planes=0), dict(planes=3), dict(a_lo=None), dict(n=n - 64),
            dict(k=k - 32), dict(lda=lda + 4), dict(a_hi=hi.data_ptr() + 8), dict(a_lo=lo.data_ptr() + 8),
            dict(w=w.data_ptr() + 8), dict(y=None), dict(epi=SILU, y=None), dict(epi=3), dict(slab, slab=None),
            dict(slab, ksplit=0)]
    bad = [dict(kernel=kernel, **b) for kernel in (2, 3) for b in both]
    bad += [dict(kernel=2, **dict(slab, ksplit=3)),            # 256 % (3 x 64)
            dict(kernel=2, stream_k=1), dict(kernel=2, **l8), dict(kernel=4), dict(kernel=0), dict(kernel=3, stream_k=2)]
    bad += [dict(kernel=3, **b) for b in (
        dict(k=64), dict(slab, ksplit=3), dict(l8, planes=1), dict(l8, w8=None), dict(l8, w8=w8.data_ptr() + 8),
        dict(l8, k=192), dict(l8, **dict(slab, ksplit=3)), dict(l8, **dict(silu, y_lo=None)),
        dict(l8, epi=SILU, y=P["y"]), dict(silu, ldy=ldy + 4), dict(silu, y_hi=P["y_hi"] + 8),
        dict(silu, y_lo=P["y_lo"] + 8), dict(n=384))]
    for b in bad:
        a = dict(base, **b)
        with pytest.raises(_lib.LlmiError):
            ops.debug_gemm_plan(**a)
        with pytest.raises(_lib.LlmiError):
            ops.debug_gemm(**a)
    # the forms the mutations start from are accepted
    for ok in (dict(kernel=2), dict(kernel=3), dict(kernel=3, **l8), dict(kernel=3, **silu), dict(kernel=2, **silu),
               dict(kernel=3, **dict(l8, **silu)), dict(kernel=2, **slab), dict(kernel=3, **slab)):
        ops.debug_gemm_plan(**dict(base, **ok))
    for v in outs.values():
        v.read()


@pytest.mark.parametrize("kernel,m,n,k,form", [(2, 300, 128, 576, 2), (3, 257, 512, 384, "lo8")])
def test_e_two_launches_are_bitwise_equal(ops, kernel, m, n, k, form):
    r, _, _ = real_run(ops, kernel, m, n, k, form, STORE, launches=2)
    same_bits(r.reads[1]["y"], r.reads[0]["y"], "the second launch")
