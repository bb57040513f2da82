"""The multi-row decode attention + o_proj of a speculative verify step (llmi_debug_attn_oproj_rows,
attn_rows.hip) against m sequential launches of the single-row pair (llmi_debug_attn_oproj) at
positions p .. p + m - 1 on copies of the same buffers. No tolerance: every row's int64 xacc,
its split partials (the whole workspace) and the raw bytes of both caches are equal.

Cache positions < p hold random finite values; positions >= p hold NaN bit patterns in both arms
before the call, so a kernel that reads a position this launch writes from the cache cannot pass.
heads 4 over 4 and over 2 kv heads, max_seq 192 (3 splits), W_o [512, 512]."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import prng  # noqa: E402

DEV = "cuda"
D, HEADS, MAX_SEQ, N_ROWS = 128, 4, 192, 512
TID = prng.layer_tid(0, prng.KIND_DOWN)
SENT = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=2)
def host_wo(wdt):
    if wdt == "i8":
        return prng.int8_weight(11, TID, N_ROWS, HEADS * D), prng.int8_row_scale(11, TID, N_ROWS)
    return prng.linear_fp16(11, TID, N_ROWS, HEADS * D), None


def raw(a):
    """The array's bytes as unsigned words (NaN patterns compare equal)."""
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def case(ops, m, p, kv_heads, cache_dt, wdt="f16", host_sized=True, seed_form="fixed"):
    rng = np.random.default_rng(1000 * p + 10 * m + kv_heads)
    kc = (rng.standard_normal((kv_heads, MAX_SEQ, D)) * 0.5).astype(cache_dt)
    vc = rng.standard_normal((kv_heads, MAX_SEQ, D)).astype(cache_dt)
    raw(kc)[:, p:] = np.iinfo(raw(kc).dtype).max  # all-ones words: NaN bit patterns from p on
    raw(vc)[:, p:] = np.iinfo(raw(vc).dtype).max
    assert np.isnan(kc[:, p:].astype(np.float32)).all() and np.isfinite(kc[:, :p].astype(np.float32)).all()
    qkv = rng.standard_normal((m, (HEADS + 2 * kv_heads) * D)).astype(np.float32)
    w, s = host_wo(wdt)
    wd, sd = T(w), None if s is None else T(s)
    seeds = rng.integers(-2 ** 40, 2 ** 40, (m, N_ROWS))
    cdt = _lib.F16 if cache_dt == np.float16 else _lib.F32
    err = T(np.zeros(1, np.int32))

    def arm(rows_call):
        kd, vd = T(kc), T(vc)
        xs, wss, rows = [], [], []
        for i in range(m):
            ws = ops.attn_workspace(HEADS, MAX_SEQ)
            ws.fill_(255)  # NaN patterns: a stale split must not leak, and untouched bytes compare equal
            x = torch.full((N_ROWS + 64,), SENT, dtype=torch.int64, device=DEV)
            a = dict(qkv=T(qkv[i]), k_cache=kd, v_cache=vd, cache_dtype=cdt, max_seq=MAX_SEQ, heads=HEADS,
                     kv_heads=kv_heads, rope=1, workspace=ws, xacc=x, w=wd, scales=sd,
                     w_dtype=_lib.I8 if wdt == "i8" else _lib.F16, n_rows=N_ROWS, ldw=HEADS * D, err=err)
            if seed_form == "zero":
                a.update(resid_fixed=T(seeds[i]), resid_scale=0.0)
            elif seed_form == "fixed" or not rows_call:
                a.update(resid_fixed=T(seeds[i]))  # (the single-row hook always seeds: the same integers)
            else:  # pre-seeded xacc: the multi-row launch seeds nothing and adds onto what is there
                x[:N_ROWS] = T(seeds[i])
            rows.append(a)
            xs.append(x)
            wss.append(ws)
        if rows_call:
            pos = T(np.array([p], np.int32))
            nact = (p + m - 1) // 64 + 1 if host_sized else 0
            ops.attn_oproj_rows([dict(a, pos_dev=pos, nact=nact) for a in rows])
        else:
            for i, a in enumerate(rows):
                ops.debug_attn_oproj(**dict(a, pos_dev=T(np.array([p + i], np.int32)),
                                            nact=(p + i) // 64 + 1 if host_sized else 0))
        xn = [N(x) for x in xs]
        for x in xn:
            assert (x[N_ROWS:] == SENT).all(), "a store past xacc's logical end"
        return [x[:N_ROWS] for x in xn], [N(ws) for ws in wss], N(kd), N(vd)

    xa, wa, ka, va = arm(False)
    xb, wb, kb, vb = arm(True)
    assert int(N(err)[0]) == 0
    for i in range(m):
        assert np.array_equal(xa[i], xb[i]), f"row {i} (position {p + i}): xacc differs"
        assert not np.array_equal(xb[i], np.where(seed_form == "zero", 0, seeds[i])), "the o_proj added nothing"
        assert np.array_equal(wa[i].view(np.uint8), wb[i].view(np.uint8)), f"row {i}: split partials differ"
    for got, ref, init in ((kb, ka, kc), (vb, va, vc)):
        assert np.array_equal(raw(got)[:, p:p + m], raw(ref)[:, p:p + m]), "cache rows p .. p + m - 1 differ"
        assert np.isfinite(got[:, p:p + m].astype(np.float32)).all()
        assert np.array_equal(raw(got)[:, :p], raw(init)[:, :p]), "a cache row below p was touched"
        assert np.array_equal(raw(got)[:, p + m:], raw(init)[:, p + m:]), "a cache row past p + m - 1 was touched"


CACHES = [np.float16, np.float32]


@pytest.mark.parametrize("cache_dt", CACHES, ids=["kv16", "kv32"])
@pytest.mark.parametrize("m,p", [(2, 0), (5, 0), (8, 0), (2, 3), (5, 3), (8, 57), (2, 63), (5, 63), (8, 63),
                                 (2, 64), (8, 64), (8, 125), (5, 125)])
@pytest.mark.parametrize("kv_heads", [4, 2], ids=["mha", "gqa"])
def test_rows_equal_sequential_launches(ops, m, p, kv_heads, cache_dt):
    """Every start position of the issue (an empty cache, 3, 57 with 8 rows ending in chunk 1, 63,
    64, 125 with rows crossing into the third chunk) and m 2, 5, 8; MHA and GQA; host-sized grid."""
    case(ops, m, p, kv_heads, cache_dt)


@pytest.mark.parametrize("cache_dt", CACHES, ids=["kv16", "kv32"])
@pytest.mark.parametrize("m,p,kv_heads", [(5, 0, 4), (8, 57, 2), (2, 63, 4), (8, 125, 2)])
def test_rows_grid_sized_for_max_seq(ops, m, p, kv_heads, cache_dt):
    """nact 0: both arms size the grid for max_seq and take the split counts from the position."""
    case(ops, m, p, kv_heads, cache_dt, host_sized=False)


@pytest.mark.parametrize("cache_dt", CACHES, ids=["kv16", "kv32"])
@pytest.mark.parametrize("m,p,kv_heads", [(2, 3, 2), (8, 57, 4), (5, 64, 2), (8, 125, 4)])
def test_rows_int8_w_o(ops, m, p, kv_heads, cache_dt):
    case(ops, m, p, kv_heads, cache_dt, wdt="i8")


@pytest.mark.parametrize("cache_dt", CACHES, ids=["kv16", "kv32"])
@pytest.mark.parametrize("seed_form", ["zero", "preseeded"])
@pytest.mark.parametrize("m,p", [(5, 3), (8, 57)])
def test_rows_seeding_forms(ops, m, p, seed_form, cache_dt):
    """resid_scale 0 (zeros) and a pre-seeded xacc (no seed written; the single-row arm seeds the
    same integers through resid_fixed); resid_fixed is every other test's form."""
    case(ops, m, p, 4, cache_dt, seed_form=seed_form)


def test_rows_argument_errors(ops):
    z = T(np.zeros((HEADS + 8) * D, np.float32))
    w, _ = host_wo("f16")
    kd = T(np.zeros((4, MAX_SEQ, D), np.float16))
    k2 = T(np.zeros((4, MAX_SEQ, D), np.float16))
    err = T(np.zeros(1, np.int32))
    pos = T(np.zeros(1, np.int32))

    def row(**over):
        x = torch.full((N_ROWS,), SENT, dtype=torch.int64, device=DEV)
        a = dict(qkv=z, k_cache=kd, v_cache=kd, cache_dtype=_lib.F16, max_seq=MAX_SEQ, pos_dev=pos, nact=1,
                 heads=HEADS, kv_heads=4, rope=1, workspace=ops.attn_workspace(HEADS, MAX_SEQ), xacc=x,
                 resid_fixed=T(np.zeros(N_ROWS, np.int64)), w=T(w), w_dtype=_lib.F16, n_rows=N_ROWS, ldw=HEADS * D,
                 err=err)
        a.update(over)
        return a

    L = _lib.lib()

    def rc(rows):
        arr = (_lib.DebugAttnOprojArgs * len(rows))()
        for i, f in enumerate(rows):
            arr[i] = ops._debug_args(_lib.DebugAttnOprojArgs, dict(f, resid_scale=1.0))
        return L.llmi_debug_attn_oproj_rows(arr, len(rows), None), rows

    wshare = T(w)
    for n in (1, 9):
        code, rows = rc([row(w=wshare) for _ in range(n)])
        assert code == -1, n                                  # LLMI_EINVAL
        assert all((N(r["xacc"]) == SENT).all() for r in rows)
    code, rows = rc([row(w=wshare), row(w=wshare, k_cache=k2)])  # the rows disagree on the cache
    assert code == -1 and all((N(r["xacc"]) == SENT).all() for r in rows)
    k8 = T(np.zeros((4, MAX_SEQ, D), np.int8))
    sc = T(np.zeros((4, MAX_SEQ), np.float16))
    code, rows = rc([row(w=wshare, k_cache=k8, v_cache=k8, cache_dtype=_lib.I8, k_scale=sc, v_scale=sc)
                     for _ in range(2)])
    assert code == -2 and b"int8" in L.llmi_last_error()      # LLMI_EUNSUPPORTED
    assert all((N(r["xacc"]) == SENT).all() for r in rows)
    assert int(N(err)[0]) == 0
