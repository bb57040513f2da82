"""Numpy restatement of the W4A16 format (LLMI_I4; include/llmi.h, llmi_quantize_groups_i4).

For a weight matrix W [rows, k] with k % 128 == 0:
  Groups: 128 consecutive columns of one row.
  Scales: one fp16 scale per (row, group), layout s [rows][k / 128], row-major, in a separate
    array.
  Values: q lies in [-7, 7] and is stored as the nibble q + 8, two nibbles per byte, the low
    nibble holding the even column; a 16-byte chunk is 32 consecutive columns and a row is
    k / 2 bytes. The quantiser never writes nibble 0; the kernel decodes nibble 0 as -8.
  Definition (bit-exact against a numpy restatement):
    amax = max |w| over the group;
    s = fp16_rne(fp32(amax / 7)), an fp16 zero becomes 2^-24, an overflow becomes 65504;
    q = clip(rint(fp32(w / fp32(s))), -7, 7), divisions correctly rounded fp32, rint
      round-half-even.
    A row holding a NaN or an infinity gets q = 0 (nibble 8) and s = 0 in every group, and
    counts once in bad_rows.
"""
import numpy as np

GROUP = 128


def pack(q):
    """int values in [-8, 7], [rows, k] -> bytes uint8 [rows, k / 2] (nibble q + 8, low = even column)."""
    n = (np.asarray(q).astype(np.int16) + 8).astype(np.uint8)
    assert n.shape[1] % 2 == 0 and n.max(initial=0) <= 15
    return (n[:, 0::2] | (n[:, 1::2] << 4)).astype(np.uint8)


def unpack(b):
    """bytes uint8 [rows, k / 2] -> int8 [rows, k] in [-8, 7]."""
    b = np.asarray(b, np.uint8)
    q = np.empty((b.shape[0], b.shape[1] * 2), np.int8)
    q[:, 0::2] = (b & 0x0F).astype(np.int8) - 8
    q[:, 1::2] = (b >> 4).astype(np.int8) - 8
    return q


def quant_i4_ref(w, row_len=None):
    """fp32 [rows, ld] (row_len data columns) -> (q int8 [rows, row_len] in [-7, 7], scale bits
    uint16 [rows, row_len / 128], bad row count)."""
    w = np.asarray(w, np.float32)
    row_len = w.shape[1] if row_len is None else row_len
    assert row_len % GROUP == 0
    rows, ng = w.shape[0], row_len // GROUP
    data = w[:, :row_len]
    bad = ~np.isfinite(data).all(axis=1)
    safe = np.where(bad[:, None], np.float32(0), data).reshape(rows, ng, GROUP)
    amax = np.abs(safe).max(axis=2).astype(np.float32)
    with np.errstate(over="ignore"):
        s = (amax / np.float32(7.0)).astype(np.float32).astype(np.float16)
    bits = s.view(np.uint16).copy()
    bits[bits == 0] = 1            # 2^-24, the smallest fp16 subnormal
    bits[bits == 0x7C00] = 0x7BFF  # 65504
    sf = bits.view(np.float16).astype(np.float32)
    ratio = (safe / sf[:, :, None]).astype(np.float32)
    q = np.clip(np.rint(ratio), -7, 7).astype(np.int8).reshape(rows, row_len)
    q[bad] = 0
    bits[bad] = 0
    return q, bits, int(bad.sum())


def dequant(q, scale_bits, dtype=np.float32):
    """q int [rows, k], scale bits uint16 (or fp16) [rows, k / 128] -> q * s, exact in `dtype`
    (a 4-bit integer times an fp16 value has at most 15 significant bits)."""
    s = np.asarray(scale_bits)
    s = s.view(np.float16) if s.dtype == np.uint16 else s.astype(np.float16)
    return np.asarray(q).astype(dtype) * np.repeat(s.astype(dtype), GROUP, axis=1)
