"""Batch option "batch_attn" (csrc/attn_batch.hip behind Batch::record_step): three slots of the `tiny`
preset with prompts of different lengths, 70 steps at max_seq 128 -- slots 0 and 1 cross the split
boundary at position 64, slot 2 is reset and given a new prompt after 40 steps, so one launch holds
slots with different split counts. Option on against option off in one batch: every slot's tokens,
final logits and cache rows, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, MAX_SEQ = 20240607, 128


def _prompt(i, n):
    from llmi.engine import synth_prompt
    return synth_prompt(3000 + i, n, 32000)


def _run(b, on, use_graph, kv):
    b.set_option("batch_attn", on)
    for i in range(3):
        b.reset(i)
    for i, n in enumerate((5, 60, 17)):
        b.set_prompt(i, _prompt(i, n))
    b.decode(40, use_graph)
    b.reset(2)
    b.set_prompt(2, _prompt(3, 9))
    b.decode(30, use_graph)
    out = []
    for i, rows in enumerate(((0, 63, 64, 69), (0, 63, 64, 69), (0, 9, 23, 29))):  # (slot 2: rows of the restart)
        out += [b.tokens(i), np.ascontiguousarray(b.logits(i)).view(np.uint32)]
        for layer in (0, 1):
            for pos in rows:
                for v in (False, True):
                    out += list(b.kv_slot_q8(i, layer, pos, v)) if kv == "I8" else [b.kv_slot(i, layer, pos, v).view(np.uint32)]
    return out


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kv", ["F16", "I8"])
def test_option_on_is_bitwise_option_off(kv, use_graph):
    import llmi
    from llmi.engine import Batch, preset
    with Batch(preset("tiny", max_seq=MAX_SEQ, kv_dtype=getattr(llmi, kv)), 3) as b:
        b.load_synthetic(SEED)
        off = _run(b, 0, use_graph, kv)
        on = _run(b, 1, use_graph, kv)
        assert len(off[0]) >= 70
        for j, (x, y) in enumerate(zip(on, off)):
            assert np.array_equal(x, y), f"output {j} differs between batch_attn 1 and 0"


def test_bad_value_raises_and_leaves_the_batch_usable():
    from llmi import _lib
    from llmi.engine import Batch, preset
    with Batch(preset("tiny", max_seq=MAX_SEQ), 2) as b:
        b.load_synthetic(SEED)
        with pytest.raises(_lib.LlmiError, match="batch_attn"):
            b.set_option("batch_attn", 2)
        b.set_option("batch_attn", 1)
        assert all(len(t) == 6 for t in b.generate([_prompt(0, 4), _prompt(1, 7)], 6))
