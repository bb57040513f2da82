"""llmi_logprobs (csrc/logprob.hip) against the float64 restatement tests/logprob_ref.py: every
value within the derived tolerance (logprob_ref.tolerance: vocab * 2^-33 + 2^-17 +
|lp| * 2^-23), the top-n ids equal with no tolerance, bits identical between launches and
between a row launched alone and as one of 8, at the smallest shapes where the kernel can go
wrong: vocab 1, odd and misaligned rows (scalar loads), the last LDS-resident size and the
first of the recompute path, the largest size, and the non-finite rows."""
import numpy as np
import pytest

import logprob_ref as L

pytestmark = pytest.mark.gpu

KINDS = ("normal", "flat", "dominant", "equal", "mixed", "only_minus_inf", "two_plus_inf", "normal2")


def _torch():
    import torch
    return torch


def _inputs(vocab, rows, seed):
    """rows x vocab logits, row r of kind KINDS[r % 8], and the id scored in each row."""
    rng = np.random.default_rng(seed)
    z = np.empty((rows, vocab), np.float32)
    ids = rng.integers(0, vocab, rows).astype(np.int32)
    for r in range(rows):
        kind = KINDS[r % len(KINDS)]
        row = (rng.standard_normal(vocab) * 4.0).astype(np.float32)
        if kind == "flat":
            row = (rng.standard_normal(vocab) * 1e-3).astype(np.float32)
        elif kind == "dominant":  # every other weight underflows to 0; their logprobs stay finite
            row = rng.standard_normal(vocab).astype(np.float32)
            row[vocab // 3] += np.float32(1e4)
        elif kind == "equal":
            row[:] = np.float32(0.625)
        elif kind == "mixed":
            row[1::5] = np.nan
            row[2::7] = -np.inf
            if vocab > 3:
                row[3::max(4, vocab // 3)] = np.inf
        elif kind == "only_minus_inf":
            row[:] = -np.inf
        elif kind == "two_plus_inf":
            row[[vocab // 4, (3 * vocab) // 4]] = np.inf
            ids[r] = vocab // 4
        z[r] = row
    return z, ids


def _launch(z, ids, n_top):
    torch = _torch()
    from llmi import ops
    zd = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    idd = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    lp, tids, tlp, lse = ops.logprobs(zd, idd, n_top)
    torch.cuda.synchronize()
    assert np.array_equal(zd.cpu().numpy().view(np.uint32), np.ascontiguousarray(z).view(np.uint32)), "logits were modified"
    return (None if lp is None else lp.cpu().numpy()), tids.cpu().numpy(), tlp.cpu().numpy(), lse.cpu().numpy()


def _check(z, ids, n_top, got):
    lp, tids, tlp, lse = got
    rows, vocab = z.shape
    assert tids.shape == (rows, n_top) and tlp.shape == (rows, n_top)
    for r in range(rows):
        kind = KINDS[r % len(KINDS)]
        want, want_lse = L.logprobs(z[r])
        L.assert_close(lp[r:r + 1], want[ids[r]:ids[r] + 1], vocab, f"V {vocab} row {r} {kind} id")
        L.assert_close(lse[r:r + 1], np.array([want_lse]), vocab, f"V {vocab} row {r} {kind} lse")
        wi, wl = L.top_n(z[r], n_top)
        np.testing.assert_array_equal(tids[r], wi, err_msg=f"V {vocab} row {r} {kind} top ids")
        L.assert_close(tlp[r], wl, vocab, f"V {vocab} row {r} {kind} top")
        if kind == "equal":
            np.testing.assert_array_equal(tids[r][:min(n_top, vocab)], np.arange(min(n_top, vocab)))
        if kind == "dominant" and vocab > 1:
            assert np.isfinite(lp[r]) and (ids[r] == vocab // 3 or lp[r] < -9e3)


# vocab 7 with 3 rows: rows 1 and 2 start 28 and 56 bytes in (scalar head / tail loads);
# 32768 is the last LDS-resident size, 32769 the first recomputing one, 131072 the largest
@pytest.mark.parametrize("vocab,rows,n_top", [
    (1, 1, 0), (1, 3, 1), (1, 8, 8), (7, 3, 0), (7, 3, 1), (7, 8, 8), (5, 3, 8), (1000, 1, 0), (1000, 3, 1), (1000, 8, 8),
    (32000, 8, 8), (32768, 8, 8), (32768, 3, 0), (32769, 8, 8), (32769, 1, 1), (131072, 8, 8), (131072, 3, 0)])
def test_values_and_top_n_match_the_restatement(vocab, rows, n_top):
    z, ids = _inputs(vocab, rows, 1000 + vocab)
    got = _launch(z, ids, n_top)
    _check(z, ids, n_top, got)
    if n_top > vocab:  # padding
        assert (got[1][:, vocab:] == -1).all() and np.isneginf(got[2][:, vocab:]).all()
    if vocab == 1:
        assert (got[0] == 0.0).all()


@pytest.mark.parametrize("vocab", [7, 1000, 32768, 32769, 131072])
def test_bits_repeat_and_do_not_depend_on_the_launch_shape(vocab):
    z, ids = _inputs(vocab, 8, 77 + vocab)
    a = _launch(z, ids, 8)
    b = _launch(z, ids, 8)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for r in range(8):  # alone (aligned, its own launch) == as row r of 8
        one = _launch(z[r:r + 1], ids[r:r + 1], 8)
        for x, y in zip(one, a):
            assert np.array_equal(x[0].view(np.uint32), y[r].view(np.uint32)), (vocab, r)


def test_without_ids_only_the_top_and_the_logsumexp_are_written():
    z, ids = _inputs(1000, 3, 5)
    lp, tids, tlp, lse = _launch(z, None, 4)
    assert lp is None
    full = _launch(z, ids, 4)
    for x, y in zip((tids, tlp, lse), full[1:]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_graph_capture_gives_the_eager_bits():
    torch = _torch()
    from llmi import ops
    z, ids = _inputs(32000, 3, 9)
    eager = _launch(z, ids, 8)
    zd, idd = torch.from_numpy(z).cuda(), torch.from_numpy(ids).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.logprobs(zd, idd, 8)  # warm: the kernel attribute is set outside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = ops.logprobs(zd, idd, 8)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))


def test_bad_arguments():
    torch = _torch()
    from llmi import ops
    from llmi._lib import LlmiError, call
    z = torch.zeros(2, 16, device="cuda")
    ids = torch.tensor([0, 15], dtype=torch.int32, device="cuda")
    for n_top in (-1, 9):
        with pytest.raises(LlmiError, match=r"failed \(-1\).*n_top must be in \[0, 8\]"):
            ops.logprobs(z, ids, n_top)
    for bad in ([0, 16], [-1, 3]):
        with pytest.raises(LlmiError, match=r"failed \(-1\).*ids must be in \[0, vocab\)"):
            ops.logprobs(z, torch.tensor(bad, dtype=torch.int32, device="cuda"), 0)
    out = torch.zeros(2, device="cuda")
    with pytest.raises(LlmiError, match=r"failed \(-1\).*null logits"):
        call("llmi_logprobs", None, 2, 16, None, 0, out.data_ptr(), None, None, None, None)
    with pytest.raises(LlmiError, match=r"failed \(-1\).*ids without out_lp"):
        call("llmi_logprobs", z.data_ptr(), 2, 16, ids.data_ptr(), 0, None, None, None, None, None)
    with pytest.raises(LlmiError, match=r"failed \(-1\).*needs top_ids and top_lp"):
        call("llmi_logprobs", z.data_ptr(), 2, 16, None, 2, None, None, None, None, None)
    with pytest.raises(LlmiError, match=r"failed \(-1\).*rows must be in \[1, 65536\]"):
        call("llmi_logprobs", z.data_ptr(), 0, 16, None, 0, None, None, None, out.data_ptr(), None)
    with pytest.raises(LlmiError, match=r"failed \(-2\).*vocab above 131072"):
        ops.logprobs(torch.zeros(1, 131073, device="cuda"), None, 0)
