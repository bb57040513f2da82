"""Host side of the fork (llmi_batch_fork, llmi_kv_copy_rows): the prototypes the Python binding
declares, null handles, and the operator's argument checks, which run before any launch -- with
n_rows = 0 an accepted call launches nothing, so made-up addresses are never touched and the whole
table runs without a GPU."""
import ctypes as C

from llmi import _lib

_P, _I = C.c_void_p, C.c_int
F32, F16, I8 = _lib.F32, _lib.F16, _lib.I8


def test_prototypes():
    L = _lib.lib()
    # int llmi_batch_fork(llmi_batch* b, int src, const int* dst, int n_dst, int keep, const int32_t* ids, int n)
    assert list(L.llmi_batch_fork.argtypes) == [_P, _I, _P, _I, _I, _P, _I]
    # int llmi_kv_copy_rows(src_k, src_v, src_k_scale, src_v_scale, dst_k, dst_v, dst_k_scale, dst_v_scale,
    #                       n_dst, cache_dtype, layers, kv_heads, max_seq, head_dim, n_rows, stream)
    assert list(L.llmi_kv_copy_rows.argtypes) == [_P] * 8 + [_I] * 7 + [_P]
    assert L.llmi_batch_fork.restype is _I and L.llmi_kv_copy_rows.restype is _I
    assert {"llmi_batch_fork", "llmi_kv_copy_rows"} <= set(_lib.header_functions())


def test_null_batch_is_an_argument_error():
    L = _lib.lib()
    dst = (C.c_int * 1)(1)
    assert L.llmi_batch_fork(None, 0, dst, 1, 0, None, 0) == -1
    assert b"[llmi][ERROR]" in L.llmi_last_error()


def _copy(n_dst=2, dtype=F16, n_rows=0, max_seq=64, head_dim=128, src=(0x1000, 0x2000), dst_k=(0x3000, 0x5000),
          dst_v=(0x4000, 0x6000), src_s=(None, None), dst_ks=None, dst_vs=None, layers=2, kv_heads=2):
    def arr(ps):
        return None if ps is None else (_P * max(len(ps), 1))(*ps)
    return _lib.lib().llmi_kv_copy_rows(src[0], src[1], src_s[0], src_s[1], arr(dst_k), arr(dst_v), arr(dst_ks),
                                        arr(dst_vs), n_dst, dtype, layers, kv_heads, max_seq, head_dim, n_rows, None)


def test_kv_copy_rows_argument_checks():
    assert _copy() == 0                       # accepted, and n_rows 0 launches nothing
    assert _copy(dtype=F32) == 0
    for bad in (dict(n_dst=0), dict(n_dst=8, dst_k=(0x3000,) * 8, dst_v=(0x4000,) * 8), dict(n_rows=-1),
                dict(n_rows=65), dict(head_dim=64), dict(dtype=_lib.I32), dict(layers=0), dict(max_seq=0),
                dict(src=(None, 0x2000)), dict(dst_k=(0x3000, None)), dict(dst_k=None),
                dict(src=(0x1008, 0x2000)), dict(dst_v=(0x4000, 0x6004)),          # not 16-byte aligned
                dict(dst_k=(0x3000, 0x1000)), dict(dst_v=(0x2000, 0x6000)),        # a destination is the source
                dict(dst_k=(0x3000, 0x2000)),                                      # ... the other source buffer
                dict(dst_k=(0x3000, 0x3000)), dict(dst_v=(0x4000, 0x4000)),        # a destination twice
                dict(dst_k=(0x3000, 0x4000))):                                     # ... as a K and as a V
        assert _copy(**bad) == -1, bad
        assert b"kv_copy_rows" in _lib.lib().llmi_last_error()
    scales = dict(dtype=I8, src_s=(0x7000, 0x8000), dst_ks=(0x9000, 0xB000), dst_vs=(0xA000, 0xC000))
    assert _copy(**scales) == 0
    for bad in (dict(src_s=(None, None)), dict(src_s=(0x7000, None)), dict(dst_ks=None), dict(dst_vs=(0xA000, None)),
                dict(dst_ks=(0x9000, 0x7000)), dict(dst_vs=(0xA000, 0xA000)), dict(dst_ks=(0x9002, 0xB000))):
        assert _copy(**dict(scales, **bad)) == -1, bad
    # the scales of another dtype are ignored
    assert _copy(dtype=F16, src_s=(None, 0x10), dst_ks=(0x9000, 0x9000)) == 0
