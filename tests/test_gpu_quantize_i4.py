"""W4A16 quantiser: llmi_quantize_groups_i4 (quant.hip) bit for bit -- the q bytes and the scale
bits -- against the numpy restatement tests/i4_ref.py (the format's definition, worded as in
include/llmi.h)."""
import numpy as np
import pytest

import i4_ref

pytestmark = pytest.mark.gpu


def _gpu_quant(w, row_len=None):
    """w fp32 [rows, ld] -> (bytes uint8 [rows, row_len / 2], scale bits uint16 [rows, row_len / 128], bad)."""
    import torch
    from llmi._lib import call
    rows, ld = w.shape
    row_len = ld if row_len is None else row_len
    wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    q = torch.full((rows, row_len // 2), 0x5A, device="cuda", dtype=torch.uint8)
    s = torch.full((rows, row_len // 128), 3.0, device="cuda", dtype=torch.float16)
    cnt = torch.zeros(1, device="cuda", dtype=torch.int32)
    call("llmi_quantize_groups_i4", wd.data_ptr(), ld, rows, row_len, q.data_ptr(), s.data_ptr(), cnt.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return q.cpu().numpy(), s.cpu().numpy().view(np.uint16), int(cnt.item())


PLANTS = ("zeros", "negzero", "tiny", "huge", "negmax", "half")


def _plant(g, kind, rng):
    """Edge values into one group (a view of 128 columns)."""
    if kind == "zeros":
        g[:] = 0.0
    elif kind == "negzero":
        g[1] = -0.0
    elif kind == "tiny":  # amax / 7 far below half the smallest fp16 subnormal: the 2^-24 floor
        g[:] = np.where(rng.random(128) < 0.5, -1e-10, 1e-10)
    elif kind == "huge":  # the scale saturates at 65504, q clamps to +-7
        g *= 1e5
        g[0], g[1] = 1e9, -1e9
    elif kind == "negmax":
        g[2] = -2.0 * np.abs(g).max() - 1.0
    elif kind == "half":  # s = 3.5 / 7 = 0.5 exactly; the rest sit on (j + 0.5) * s
        j = (np.arange(128) % 13) - 6
        g[:] = (j + 0.5) * 0.5
        g[0] = 3.5


# (rows, row_len, ld): the issue's shapes, one with ld > row_len, and the launcher's thresholds
# (rows up to 4096 and up to 16384 columns are kept in registers, longer ones are read twice):
# each boundary and the first size behind it
CASES = [(3, 128, 128), (5, 512, 512), (2, 11008, 11008), (2, 13824, 13824), (3, 16384, 16384),
         (3, 768, 776), (2, 4096, 4096), (2, 4224, 4228), (2, 16512, 16512)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_bit_exact(case):
    rows, row_len, ld = CASES[case]
    ng = row_len // 128
    rng = np.random.default_rng(200 + case)
    w = rng.standard_normal((rows, ld)).astype(np.float32)
    # row 0 carries the plants, each in a group of its own (as many as the row has groups); with one
    # group per row they go to different rows instead
    where = {}
    for i, kind in enumerate(PLANTS):
        r, g = (0, (i * 5 + 1) % ng) if ng >= 2 * len(PLANTS) else (i % rows, (i // rows) % ng)
        if (r, g) in where:
            continue
        where[(r, g)] = kind
        _plant(w[r, g * 128:(g + 1) * 128], kind, rng)
    if ng >= 2 * len(PLANTS):
        assert sorted(where.values()) == sorted(PLANTS)
    w[:, row_len:] = 1e30  # padding: must not move any scale
    want_q, want_s, bad = i4_ref.quant_i4_ref(w, row_len)
    assert bad == 0
    got_b, got_s, got_bad = _gpu_quant(w, row_len)
    assert got_bad == 0
    np.testing.assert_array_equal(got_s, want_s)
    np.testing.assert_array_equal(got_b, i4_ref.pack(want_q))
    assert not (got_b & 0x0F == 0).any() and not (got_b >> 4 == 0).any()  # nibble 0 is never written
    # the plants did what they are there for
    sf = want_s.view(np.float16).astype(np.float32)
    for (r, g), kind in where.items():
        qg = want_q[r, g * 128:(g + 1) * 128]
        if kind in ("zeros", "tiny"):
            assert want_s[r, g] == 1 and not qg.any()
        elif kind == "huge":
            assert want_s[r, g] == 0x7BFF and qg[0] == 7 and qg[1] == -7
        elif kind == "negmax":
            assert qg[2] == -7
        elif kind == "half":
            assert sf[r, g] == 0.5
            np.testing.assert_array_equal(qg[1:], np.rint((np.arange(1, 128) % 13) - 6 + 0.5).astype(np.int8))


def test_non_finite_rows_are_counted_and_refused():
    import torch
    from llmi import ops
    from llmi._lib import LlmiError
    rng = np.random.default_rng(6)
    w = rng.standard_normal((6, 512)).astype(np.float32)
    w[1, 300] = np.nan        # group 2 of row 1
    w[4, 3] = -np.inf         # group 0 of row 4
    want_q, want_s, bad = i4_ref.quant_i4_ref(w)
    assert bad == 2
    got_b, got_s, got_bad = _gpu_quant(w)
    assert got_bad == 2
    np.testing.assert_array_equal(got_s, want_s)
    np.testing.assert_array_equal(got_b, i4_ref.pack(want_q))
    for r in range(6):
        zero = r in (1, 4)
        assert (not got_s[r].any()) == zero and bool((got_b[r] == 0x88).all()) == zero
    with pytest.raises(LlmiError, match="NaN or an infinity") as ei:
        ops.quantizeGroupsInt4(torch.from_numpy(w).cuda())
    assert ei.value.bad_rows == 2
    w[1, 300] = w[4, 3] = 0.5
    q, s = ops.quantizeGroupsInt4(torch.from_numpy(w).cuda())
    assert q.dtype == torch.uint8 and tuple(q.shape) == (6, 256) and s.dtype == torch.float16 and tuple(s.shape) == (6, 4)
    want_q, want_s, _ = i4_ref.quant_i4_ref(w)
    np.testing.assert_array_equal(q.cpu().numpy(), i4_ref.pack(want_q))
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint16), want_s)


def test_kernel_argument_checks():
    import torch
    from llmi._lib import LlmiError, call
    w = torch.zeros(2, 264, device="cuda")
    q = torch.full((2, 132), 0x5A, device="cuda", dtype=torch.uint8)
    s = torch.zeros(2, 2, device="cuda", dtype=torch.float16)
    st = torch.cuda.current_stream().cuda_stream

    def refused(wp, ld, row_len):
        with pytest.raises(LlmiError, match="quantize_groups_i4"):
            call("llmi_quantize_groups_i4", wp, ld, 2, row_len, q.data_ptr(), s.data_ptr(), None, st)

    refused(w.data_ptr(), 264, 192)       # row_len not a multiple of 128
    refused(w.data_ptr(), 128, 256)       # row_len > ld
    refused(w.data_ptr() + 4, 260, 256)   # w not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((q == 0x5A).all()), "a refused call wrote q"
