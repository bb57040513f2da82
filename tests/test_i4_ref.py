"""The W4A16 format's numpy restatement (tests/i4_ref.py) checked against itself, on the CPU."""
import re

import numpy as np

import i4_ref
from llmi import _lib
from llmi._lib import I4  # the format's dtype: the restatement describes nothing without it


def test_pack_unpack_round_trip_with_nibble_zero():
    rng = np.random.default_rng(0)
    q = rng.integers(-8, 8, size=(5, 256)).astype(np.int8)
    q[0, :16] = np.arange(-8, 8)  # every nibble, 0 (= -8) included
    b = i4_ref.pack(q)
    assert b.dtype == np.uint8 and b.shape == (5, 128)
    # the low nibble holds the even column, value + 8
    assert b[0, 0] == ((-8 + 8) | ((-7 + 8) << 4)) and b[0, 7] == ((6 + 8) | ((7 + 8) << 4))
    np.testing.assert_array_equal(i4_ref.unpack(b), q)
    # every byte value decodes and re-encodes to itself
    allb = np.arange(256, dtype=np.uint8).reshape(1, 256)
    np.testing.assert_array_equal(i4_ref.pack(i4_ref.unpack(allb)), allb)
    assert i4_ref.unpack(np.zeros((1, 1), np.uint8)).tolist() == [[-8, -8]]


def test_requantising_a_dequantised_matrix_is_exact():
    rng = np.random.default_rng(1)
    rows, k = 6, 512
    q0 = rng.integers(-7, 8, size=(rows, k)).astype(np.int8)
    q0.reshape(rows, k // 128, 128)[:, :, 5] = np.where(rng.random((rows, k // 128)) < 0.5, -7, 7)  # a +-7 a group
    s0 = (rng.random((rows, k // 128)) * 0.05 + 1e-3).astype(np.float16)
    w = i4_ref.dequant(q0, s0)
    assert w.dtype == np.float32
    np.testing.assert_array_equal(w.astype(np.float64), i4_ref.dequant(q0, s0, np.float64))  # exact in fp32
    q, bits, bad = i4_ref.quant_i4_ref(w)
    assert bad == 0
    np.testing.assert_array_equal(bits, s0.view(np.uint16))
    np.testing.assert_array_equal(q, q0)
    assert q.min() >= -7 and not (i4_ref.pack(q) & 0x0F == 0).any() and not (i4_ref.pack(q) >> 4 == 0).any()


def test_restatement_edge_rules():
    w = np.zeros((3, 256), np.float32)
    w[0, :128] = 1e-12      # far below the fp16 subnormal floor: scale 2^-24, q 0
    w[0, 128:] = 1e9        # the scale saturates at 65504, q clamps to 7
    w[1, 7] = np.nan
    w[2, 128:] = (np.arange(128) % 13 - 6 + 0.5) * 0.5   # exact halves of s = 0.5
    w[2, 128] = 3.5
    q, bits, bad = i4_ref.quant_i4_ref(w)
    assert bad == 1 and not q[1].any() and not bits[1].any()
    assert bits[0, 0] == 1 and not q[0, :128].any()
    assert bits[0, 1] == 0x7BFF and (q[0, 128:] == 7).all()
    assert bits[2, 1] == np.float16(0.5).view(np.uint16)
    np.testing.assert_array_equal(q[2, 129:], np.rint(np.arange(1, 128) % 13 - 6 + 0.5).astype(np.int8))


def test_dtype_value():
    import llmi
    assert I4 == 5 and _lib.I4 == 5 and llmi.I4 == 5
    assert "llmi_quantize_groups_i4" in _lib._SIGS and "llmi_quantize_groups_i4" in _lib.header_functions()


def test_header_states_the_format_in_the_restatements_words():
    """include/llmi.h documents the format word for word with tests/i4_ref.py's docstring."""
    def norm(t):
        return re.sub(r"\s+", " ", t.replace("*", " ")).strip()
    doc, header = norm(i4_ref.__doc__), norm(open(_lib.HEADER).read())
    fmt = doc[doc.index("Groups:"):doc.index("round-half-even.") + len("round-half-even.")]
    assert len(fmt) > 600 and fmt in header
    assert "A row holding a NaN or an infinity gets q = 0 (nibble 8) and s = 0 in every group" in header
