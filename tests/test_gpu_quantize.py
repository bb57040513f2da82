"""W8A16 quantise-on-load: llmi_quantize_rows_i8 (quant.hip) and the loaders built on it
(llmi_engine_load_bin_quantized / llmi_engine_load_tensor_quantized /
llmi_group_load_bin_quantized, LlamaModel::loadWeightsQuantized).

The quantiser's definition is restated here in numpy (quant_ref) and the kernel must match
it bit for bit, q and the scale bits. Per row of w [rows, ld] with row_len data columns:
  amax = max |w[r, :row_len]|                 (the whole row, whatever slice is written)
  s    = fp16_rne(fp32(amax / 127))           (fp16 zero -> 2^-24, overflow -> 65504)
  q    = clip(rint(fp32(w[r, col0:col0 + cols] / fp32(s))), -127, 127)
  a row with a NaN / infinity: s = 0, q = 0, counted in bad_rows.

End to end the engine loads fp32 .bin files of the tiny model, quantises them on the device,
and must give the tokens of the oracle run on the numpy-quantised weights exactly, with the
last logits within the project's bar (LOGIT_TOL of tests/test_gpu_engine.py, 1e-3 rel-L2)."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402
from oracle import prng  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "llm-inference_amd", "lib")
LOGIT_TOL = 1e-3  # tests/test_gpu_engine.py
OUTLIER = 8.0     # column 0 of every o_proj / down row: +-OUTLIER x the row's maximum
N_NEW = 8


# ------------------------------------------------------------------ numpy restatement
def quant_ref(w, row_len=None, col0=0, cols=None):
    """-> (q int8 [rows, cols], scale bits uint16 [rows], bad row count)."""
    w = np.asarray(w, np.float32)
    row_len = w.shape[1] if row_len is None else row_len
    cols = row_len - col0 if cols is None else cols
    data = w[:, :row_len]
    bad = ~np.isfinite(data).all(axis=1)
    safe = np.where(bad[:, None], np.float32(0), data)
    amax = np.abs(safe).max(axis=1).astype(np.float32)
    with np.errstate(over="ignore"):
        s = (amax / np.float32(127.0)).astype(np.float32).astype(np.float16)
    bits = s.view(np.uint16).copy()
    bits[bits == 0] = 1            # 2^-24, the smallest fp16 subnormal
    bits[bits == 0x7C00] = 0x7BFF  # 65504
    sf = bits.view(np.float16).astype(np.float32)
    ratio = (safe[:, col0:col0 + cols] / sf[:, None]).astype(np.float32)
    q = np.clip(np.rint(ratio), -127, 127).astype(np.int8)
    q[bad] = 0
    bits[bad] = 0
    return q, bits, int(bad.sum())


def _gpu_quant(w, row_len=None, col0=0, cols=None):
    import torch
    from llmi import ops
    q, s = ops.quantizeRowsInt8(torch.from_numpy(np.ascontiguousarray(w)).cuda(), col0=col0, cols=cols,
                                row_len=row_len)
    torch.cuda.synchronize()
    return q.cpu().numpy(), s.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------ 1. kernel, bit-exact
PLANTS = ("zeros", "negzero", "tiny", "huge", "negmax", "half", "plain")


def _plant(row, kind, rng):
    n = row.shape[0]
    if kind == "zeros":
        row[:] = 0.0
    elif kind == "negzero":
        row[1] = -0.0
    elif kind == "tiny":  # amax / 127 is far below half the smallest fp16 subnormal: the floor
        row[:] = np.where(rng.random(n) < 0.5, -1e-9, 1e-9)
    elif kind == "huge":  # the scale saturates at 65504, q clamps to +-127
        row *= 1e5
        row[0], row[1] = 1e9, -1e9
    elif kind == "negmax":
        row[2 % n] = -2.0 * np.abs(row).max() - 1.0
    elif kind == "half":  # s = 63.5 / 127 = 0.5 exactly; the rest sit on (k + 0.5) * s
        k = (np.arange(n) % 41) - 20
        row[:] = (k + 0.5) * 0.5
        row[0] = 63.5


CASES = [(3, 4, 4, 0, 4), (5, 260, 260, 0, 260), (7, 1028, 1032, 0, 1028), (7, 1028, 1032, 512, 516),
         (2, 13824, 13824, 0, 13824),
         # the launcher's row-length thresholds (4, 8 or 16 float4 per lane kept in registers; past
         # 16,384 floats the row is read twice): each boundary and the first size behind it
         (2, 4096, 4096, 0, 4096), (3, 4100, 4104, 2048, 2052), (2, 8192, 8192, 0, 8192),
         (3, 8196, 8196, 4096, 4100), (2, 16384, 16384, 0, 16384), (3, 16388, 16392, 8192, 8196)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_bit_exact(case):
    rows, row_len, ld, col0, cols = CASES[case]
    rng = np.random.default_rng(100 + case)
    w = rng.standard_normal((rows, ld)).astype(np.float32)
    kinds = [PLANTS[(r + 3 * case) % len(PLANTS)] for r in range(rows)]
    for r, kind in enumerate(kinds):
        _plant(w[r, :row_len], kind, rng)
    if rows >= len(PLANTS):
        assert set(kinds) == set(PLANTS)
    if col0 > 0:  # every row's maximum lies in front of the written slice
        for r, kind in enumerate(kinds):
            if kind in ("plain", "negzero"):
                w[r, 7] = 3.0 * np.abs(w[r, :row_len]).max() * (-1.0 if r % 2 else 1.0)
            if kind not in ("zeros", "tiny"):
                assert np.abs(w[r, :row_len]).argmax() < col0
    w[:, row_len:] = 1e30  # padding: must not move the scale
    want_q, want_s, bad = quant_ref(w, row_len, col0, cols)
    assert bad == 0
    got_q, got_s = _gpu_quant(w, row_len, col0, cols)
    assert got_q.shape == (rows, cols) and got_q.dtype == np.int8
    np.testing.assert_array_equal(got_s, want_s)
    np.testing.assert_array_equal(got_q, want_q)
    assert got_q.min() >= -127
    # the planted rows did what they are there for
    sf = want_s.view(np.float16).astype(np.float32)
    for r, kind in enumerate(kinds):
        if kind in ("zeros", "tiny"):
            assert want_s[r] == 1 and not want_q[r].any()
        elif kind == "huge":
            assert want_s[r] == 0x7BFF and (col0 > 0 or (want_q[r, 0] == 127 and want_q[r, 1] == -127))
        elif kind == "half":
            assert sf[r] == 0.5
            k = (np.arange(col0, col0 + cols) % 41) - 20
            sel = np.arange(col0, col0 + cols) != 0
            np.testing.assert_array_equal(want_q[r][sel], np.rint(k + 0.5)[sel].astype(np.int8))


def test_kernel_argument_checks():
    import torch
    from llmi import ops
    from llmi._lib import LlmiError
    w = torch.zeros(2, 16, device="cuda")
    for kw in (dict(col0=2), dict(cols=6), dict(row_len=10), dict(col0=8, cols=12), dict(row_len=20)):
        with pytest.raises(LlmiError, match="quantize_rows_i8"):
            ops.quantizeRowsInt8(w, **kw)


# ------------------------------------------------------------------ 2. idempotence
def test_requantising_w8a16_weights_is_exact():
    seed, tid, rows, cols = 11, prng.layer_tid(0, prng.KIND_GATE), 64, 512
    q0 = np.clip(prng.int8_weight(seed, tid, rows, cols), -127, 127).astype(np.int8)
    q0[:, 0] = 127
    s0 = prng.int8_row_scale(seed, tid, rows)
    w = q0.astype(np.float32) * s0.astype(np.float32)[:, None]
    rq, rs, _ = quant_ref(w)
    np.testing.assert_array_equal(rq, q0)
    np.testing.assert_array_equal(rs, s0.view(np.uint16))
    q, s = _gpu_quant(w)
    np.testing.assert_array_equal(q, q0)
    np.testing.assert_array_equal(s, s0.view(np.uint16))


# ------------------------------------------------------------------ 3. non-finite input
def test_non_finite_rows_are_counted_and_refused():
    import torch
    import llmi
    from llmi import ops
    from llmi._lib import LlmiError, call
    from llmi.engine import Engine, preset
    rng = np.random.default_rng(5)
    w = rng.standard_normal((6, 260)).astype(np.float32)
    w[1, 259] = np.nan
    w[4, 3] = -np.inf
    want_q, want_s, bad = quant_ref(w)
    assert bad == 2
    wd = torch.from_numpy(w).cuda()
    q = torch.full((6, 260), 77, device="cuda", dtype=torch.int8)
    s = torch.full((6,), 3.0, device="cuda", dtype=torch.float16)
    cnt = torch.zeros(1, device="cuda", dtype=torch.int32)
    call("llmi_quantize_rows_i8", wd.data_ptr(), 260, 6, 260, 0, 260, q.data_ptr(), s.data_ptr(), cnt.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    assert int(cnt.item()) == 2
    np.testing.assert_array_equal(q.cpu().numpy(), want_q)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint16), want_s)
    assert not q[1].any() and not q[4].any() and s[1] == 0 and s[4] == 0
    with pytest.raises(LlmiError, match="NaN or an infinity") as ei:
        ops.quantizeRowsInt8(wd)
    assert ei.value.bad_rows == 2
    name = "model.layers.1.mlp.down_proj.weight"
    down = rng.standard_normal((512, 1024)).astype(np.float32)
    down[17, 900] = np.inf
    with Engine(preset("tiny", weight_dtype=llmi.I8, kv_dtype=llmi.F32)) as e:
        with pytest.raises(LlmiError, match="layers.1.mlp.down_proj"):
            e.load_tensor(name, down, quantize=True)
        down[17, 900] = 0.0
        e.load_tensor(name, down, quantize=True)


# ------------------------------------------------------------------ 4-7. the loaders
def _with_linears(w, fn):
    """ModelWeights with every layer's four linear tensors replaced by fn(name, fp32 matrix)
    -> (matrix, scales or None)."""
    layers = []
    for lw in w.layers:
        new = {}
        for name in ("qkv", "o", "gate_up", "down"):
            new[name], new[name + "_s"] = fn(name, getattr(lw, name))
        layers.append(dataclasses.replace(lw, **new))
    return R.ModelWeights(embed=w.embed, lm_head=w.lm_head, final_norm=w.final_norm, layers=layers)


def _quantised(m):
    q, bits, bad = quant_ref(m)
    assert bad == 0
    return q, bits.view(np.float16)


def _slice_local(m, world):
    """What a rank would hold had it taken each scale from its own column slice: the
    dequantised fp32 matrix, slices side by side."""
    n = m.shape[1] // world
    parts = []
    for r in range(world):
        parts.append(R.dequant(*_quantised(np.ascontiguousarray(m[:, r * n:(r + 1) * n]))))
    return np.concatenate(parts, axis=1)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    import llmi
    from llmi import convert as CV
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)
    seed = int(f["seed"])
    cfg = R.LlamaConfig(hidden=512, heads=4, kv_heads=4, inter=1024, layers=2, max_seq=64)
    base = R.make_model_weights(cfg, seed)

    def fp32_with_outliers(name, m):
        m = np.array(m, dtype=np.float32)
        if name in ("o", "down"):
            sign = np.where(np.arange(m.shape[0]) % 2 == 0, 1.0, -1.0).astype(np.float32)
            m[:, 0] = sign * np.float32(OUTLIER) * np.abs(m).max(axis=1)
        return m, None

    w32 = _with_linears(base, fp32_with_outliers)
    t = {"model.embed_tokens.weight": w32.embed, "lm_head.weight": w32.lm_head, "model.norm.weight": w32.final_norm}
    for l, L in enumerate(w32.layers):
        p = f"model.layers.{l}."
        t.update({p + "input_layernorm.weight": L.attn_norm, p + "post_attention_layernorm.weight": L.ffn_norm,
                  p + "self_attn.qkv.weight": L.qkv, p + "self_attn.o_proj.weight": L.o,
                  p + "mlp.gate_up_proj.weight": L.gate_up, p + "mlp.down_proj.weight": L.down})
    prefix = str(tmp_path_factory.mktemp("qbin")) + "/"
    CV.write_bin(prefix, t)
    prompt = np.asarray(f["prompt"], np.int32)
    wq = _with_linears(w32, lambda name, m: _quantised(m))
    toks, logits = R.LlamaOracle(cfg, weights=wq).greedy(prompt, N_NEW)
    # the quantisation is visible at the bar's scale: the unquantised model is further away
    _, logits32 = R.LlamaOracle(cfg, weights=w32).greedy(prompt, N_NEW)
    d32 = _rel(logits32, logits)
    print(f"oracle: unquantised vs quantised logits rel-L2 {d32:.3e}")
    assert d32 > 2 * LOGIT_TOL
    llmi.lib()
    return dict(cfg=cfg, w32=w32, prefix=prefix, prompt=prompt, tokens=toks, logits=logits)


def _i8_cfg():
    import llmi
    from llmi.engine import preset
    return preset("tiny", weight_dtype=llmi.I8, kv_dtype=llmi.F32)


@pytest.mark.parametrize("prefill", [False, True])
def test_engine_load_bin_quantized_matches_oracle(tiny, prefill):
    from llmi.engine import Engine
    with Engine(_i8_cfg()) as e:
        e.load_bin(tiny["prefix"], quantize=True)
        toks = e.generate(tiny["prompt"], N_NEW, prefill=prefill)
        logits = e.logits()
    r = _rel(logits, tiny["logits"])
    print(f"int8 engine, quantised on load (prefill={prefill}): logits rel-L2 vs oracle {r:.3e}")
    np.testing.assert_array_equal(toks, tiny["tokens"])
    assert r < LOGIT_TOL


def test_group_load_bin_quantized_tp2_keeps_full_row_scales(tiny):
    from llmi.engine import TPGroup
    world = 2
    # a rank that took the maximum over its own column slice of o_proj / down would be this model
    local = _with_linears(tiny["w32"], lambda name, m: (_slice_local(m, world), None) if name in ("o", "down")
                          else _quantised(m))
    ltoks, llogits = R.LlamaOracle(tiny["cfg"], weights=local).greedy(tiny["prompt"], N_NEW)
    gap = _rel(llogits, tiny["logits"])
    print(f"oracle: slice-local scales vs full-row scales, logits rel-L2 {gap:.3e}")
    assert gap > 2e-3  # if the inputs change and this weakens, raise OUTLIER; the bar below stays
    with TPGroup(_i8_cfg(), world) as g:
        g.load_bin(tiny["prefix"], quantize=True)
        toks = g.generate(tiny["prompt"], N_NEW)
        logits = g.logits()
    r = _rel(logits, tiny["logits"])
    print(f"int8 TP=2 group, quantised on load: logits rel-L2 vs oracle {r:.3e}")
    np.testing.assert_array_equal(toks, tiny["tokens"])
    assert r <= LOGIT_TOL


def test_quantised_load_errors(tiny):
    import llmi
    from llmi._lib import LlmiError
    from llmi.engine import Engine, TPGroup, preset
    with Engine(preset("tiny")) as e:
        with pytest.raises(LlmiError, match="quantize needs an int8 engine"):
            e.load_bin(tiny["prefix"], quantize=True)
        with pytest.raises(LlmiError, match="quantize needs an int8 engine"):
            e.load_tensor("model.norm.weight", np.ones(512, np.float32), quantize=True)
    with TPGroup(preset("tiny", kv_dtype=llmi.F32), 2) as g:
        with pytest.raises(LlmiError, match="quantize needs an int8 engine"):
            g.load_bin(tiny["prefix"], quantize=True)
    with Engine(_i8_cfg()) as e:
        with pytest.raises(LlmiError, match="int8.*quantized"):
            e.load_bin(tiny["prefix"])
        with pytest.raises(LlmiError, match="expected"):
            e.load_tensor("model.layers.0.self_attn.o_proj.weight", np.ones(12, np.float32), quantize=True)


def test_cpp_load_weights_quantized(tiny, tmp_path):
    exe = str(tmp_path / "test_quantized_load")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "test_quantized_load.cpp"), "-L", LIBDIR, "-lllmi",
           f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [exe, tiny["prefix"], str(N_NEW)] + [str(int(t)) for t in tiny["prompt"]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = next(json.loads(l) for l in r.stdout.splitlines() if l.startswith("{"))
    np.testing.assert_array_equal(out["tokens"], tiny["tokens"])
    assert out["plain_refused"] is True and len(out["factory_tokens"]) == N_NEW
