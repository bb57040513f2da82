"""ops.kv_copy_rows (llmi_kv_copy_rows, csrc/kv_fork.hip) alone, against numpy slicing, byte for
byte: rows [0, n_rows) of every (layer, kv head) of a K and a V cache -- and of the int8 cache's
fp16 scales -- go to 1, 2 or 7 destinations in one launch; every other byte of a destination keeps
its sentinel and the source is unchanged. No tolerance: np.array_equal on the raw bytes of whole
buffers.

Shapes: layers 2, kv_heads 2, head_dim 128; max_seq 192, and for the int8 cache also 68, where
the scale segments start 8-byte- but not 16-byte-aligned (68 * 2 = 136 bytes apart). n_rows 0, 1,
63, 64, 65 and max_seq: nothing, one row, around the 64-row boundary (an fp32 segment of 64 rows is
two full 16 KiB work items, 65 rows a third, partial one), everything. Every case runs eagerly and
once more captured in a graph and replayed (n_rows 0 launches nothing, so there is nothing to
capture: eager only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYERS, KV_HEADS, D = 2, 2, 128
SENTINEL = 0xA5
CONFIGS = [("f32", 192), ("f16", 192), ("i8", 192), ("i8", 68)]


def _torch_dtype(name):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "i8": torch.int8}[name]


def _random_bytes(shape, dtype, seed):
    """A device tensor of this shape and dtype holding random bytes (every bit pattern, NaNs too)."""
    import torch
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator(device="cpu").manual_seed(seed)
    raw = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).cuda()
    return raw.view(dtype).view(shape)


def _sentinel(shape, dtype):
    import torch
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).view(shape)


def _bytes(t):
    import torch
    return t.contiguous().view(-1).view(torch.uint8).cpu().numpy().reshape(*t.shape[:3], -1)


class _Case:
    """One source (K, V and, int8, their scales) and n_dst sentinel-filled destinations."""

    def __init__(self, dtype, max_seq, n_dst, seed=0):
        import torch
        self.q8 = dtype == "i8"
        self.max_seq, self.n_dst = max_seq, n_dst
        td = _torch_dtype(dtype)
        self.shape, self.sshape = (LAYERS, KV_HEADS, max_seq, D), (LAYERS, KV_HEADS, max_seq)
        self.src = [_random_bytes(self.shape, td, seed + i) for i in range(2)]
        self.src_s = [_random_bytes(self.sshape, torch.float16, seed + 2 + i) for i in range(2)] if self.q8 else None
        self.src_bytes = [_bytes(t) for t in self.src + (self.src_s or [])]
        self.td = td
        self.refill()

    def refill(self):
        import torch
        self.dst = [[_sentinel(self.shape, self.td) for _ in range(self.n_dst)] for _ in range(2)]
        self.dst_s = ([[_sentinel(self.sshape, torch.float16) for _ in range(self.n_dst)] for _ in range(2)]
                      if self.q8 else None)

    def run(self, n_rows):
        from llmi import ops
        kw = {}
        if self.q8:
            kw = dict(src_k_scale=self.src_s[0], src_v_scale=self.src_s[1], dst_k_scale=self.dst_s[0],
                      dst_v_scale=self.dst_s[1])
        ops.kv_copy_rows(self.src[0], self.src[1], self.dst[0], self.dst[1], n_rows, **kw)

    def check(self, n_rows, what):
        import torch
        torch.cuda.synchronize()
        groups = [self.dst[0], self.dst[1]] + (self.dst_s if self.q8 else [])
        for w, (srcb, dsts) in enumerate(zip(self.src_bytes, groups)):
            want = np.full_like(srcb, SENTINEL)
            want[:, :, :n_rows] = srcb[:, :, :n_rows]
            for d, t in enumerate(dsts):
                assert np.array_equal(_bytes(t), want), f"{what}: buffer {w} of destination {d}, n_rows {n_rows}"
        now = [_bytes(t) for t in self.src + (self.src_s or [])]
        assert all(np.array_equal(a, b) for a, b in zip(now, self.src_bytes)), f"{what}: the source changed"

    def check_untouched(self, what):
        self.check(0, what)


@pytest.mark.parametrize("n_dst", [1, 2, 7])
@pytest.mark.parametrize("dtype,max_seq", CONFIGS, ids=[f"{d}-{m}" for d, m in CONFIGS])
def test_copy_rows_eager_and_graph(dtype, max_seq, n_dst):
    import torch
    c = _Case(dtype, max_seq, n_dst)
    side = torch.cuda.Stream()
    for n_rows in (0, 1, 63, 64, 65, max_seq):
        c.refill()
        c.run(n_rows)
        c.check(n_rows, "eager")
        if n_rows == 0:
            continue
        c.refill()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                c.run(n_rows)
        c.check_untouched("captured, not replayed")
        g.replay()
        c.check(n_rows, "graph")


def _refused(c, what, **over):
    """The call with these arguments replaced returns LLMI_EINVAL and writes nothing."""
    from llmi import ops
    from llmi._lib import LlmiError
    a = dict(src_k=c.src[0], src_v=c.src[1], dst_k=c.dst[0], dst_v=c.dst[1], n_rows=5)
    if c.q8:
        a.update(src_k_scale=c.src_s[0], src_v_scale=c.src_s[1], dst_k_scale=c.dst_s[0], dst_v_scale=c.dst_s[1])
    a.update(over)
    with pytest.raises(LlmiError) as err:
        ops.kv_copy_rows(**a)
    assert "(-1)" in str(err.value) and "kv_copy_rows" in str(err.value), (what, str(err.value))
    c.check_untouched(what)


def test_einval_cases_write_nothing():
    import torch
    from llmi import _lib
    assert _lib.lib().llmi_kv_copy_rows is not None
    c = _Case("f16", 192, 2)
    _refused(c, "n_dst 0", dst_k=[], dst_v=[])
    more = [_sentinel(c.shape, c.td) for _ in range(8)]
    _refused(c, "n_dst 8", dst_k=more, dst_v=[_sentinel(c.shape, c.td) for _ in range(8)])
    _refused(c, "n_rows -1", n_rows=-1)
    _refused(c, "n_rows max_seq + 1", n_rows=193)
    _refused(c, "a destination is the source", dst_k=[c.dst[0][0], c.src[0]])
    _refused(c, "a V destination is the source", dst_v=[c.src[1], c.dst[1][1]])
    _refused(c, "a destination appears twice", dst_k=[c.dst[0][0], c.dst[0][0]])
    _refused(c, "a V destination appears twice", dst_v=[c.dst[1][1], c.dst[1][1]])
    # head_dim 64: the same bytes seen as [2, 2, 384, 64]
    as64 = lambda t: t.view(LAYERS, KV_HEADS, 384, 64)
    _refused(c, "head_dim 64", src_k=as64(c.src[0]), src_v=as64(c.src[1]), dst_k=[as64(t) for t in c.dst[0]],
             dst_v=[as64(t) for t in c.dst[1]])
    q = _Case("i8", 192, 2)
    _refused(q, "int8 without scales", src_k_scale=None, src_v_scale=None, dst_k_scale=None, dst_v_scale=None)
    _refused(q, "int8 without destination scales", dst_k_scale=None, dst_v_scale=None)
    _refused(q, "a scale destination is the source", dst_k_scale=[q.dst_s[0][0], q.src_s[0]])
    _refused(q, "a scale destination appears twice", dst_v_scale=[q.dst_s[1][0], q.dst_s[1][0]])
    # and the arguments of a refused call are fine otherwise
    c.run(5)
    c.check(5, "after the refusals")
    q.run(5)
    q.check(5, "after the refusals (int8)")
    torch.cuda.synchronize()
