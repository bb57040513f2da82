"""Batch option "rows_mfma" (llmi_batch_set_option; gemv_rows_mfma.hip behind Batch::record_step):
the option's interface, a slot's independence of its neighbours (bitwise), its distance to the
default path (LOGIT_TOL, the bar tests/test_gpu_prefill.py holds the two-plane prefill to against
the decode path), and that turning it off gives back the default path's bits. `tiny` preset,
fp16 and int8 synthetic weights, eager and captured steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, N_NEW, LOGIT_TOL = 20240607, 40, 1e-3


def _batch(wdt, n_seq=3):
    import llmi
    from llmi.engine import Batch, preset
    b = Batch(preset("tiny", max_seq=128, weight_dtype=getattr(llmi, wdt)), n_seq)
    b.load_synthetic(SEED)
    return b


def _prompt(i, n):
    from llmi.engine import synth_prompt
    return synth_prompt(2000 + i, n, 32000)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


WDT = pytest.mark.parametrize("wdt", ["F16", "I8"])
GRAPH = pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])


def test_set_option_interface():
    from llmi import _lib
    with _batch("F16", 2) as b:
        b.set_option("rows_mfma", 1)
        with pytest.raises(_lib.LlmiError, match="rows_mfma"):
            b.set_option("rows_mfma", 2)
        with pytest.raises(_lib.LlmiError, match="unknown option"):
            b.set_option("rows_wmma", 1)
        assert len(b.generate([_prompt(0, 4), None], 6)[0]) == 6  # still usable, the option on


@WDT
@GRAPH
def test_slot_does_not_depend_on_its_neighbours(wdt, use_graph):
    """Slot 0 alone, then beside two slots with other prompts of other lengths (one outlives it,
    one goes idle before it ends): the same tokens and final logits, bit for bit."""
    p0 = _prompt(0, 7)
    with _batch(wdt) as b:
        b.set_option("rows_mfma", 1)
        alone = b.generate([p0, None, None], N_NEW, use_graph=use_graph)[0]
        logits = _bits(b.logits(0))
        crowd = b.generate([p0, _prompt(1, 12), _prompt(2, 3)], N_NEW, use_graph=use_graph)
        assert np.array_equal(crowd[0], alone), (crowd[0], alone)
        assert np.array_equal(_bits(b.logits(0)), logits), "slot 0's logits depend on its neighbours"
        assert not np.array_equal(crowd[1][:8], crowd[2][:8])


@WDT
@GRAPH
def test_logits_close_to_the_default_path(wdt, use_graph):
    """A forced 12-token prompt consumed as decode steps (no sampled input) by two slots."""
    prompts = [_prompt(3, 12), _prompt(4, 12)]
    with _batch(wdt, 2) as b:
        got = {}
        for on in (0, 1):
            b.set_option("rows_mfma", on)
            for i, p in enumerate(prompts):
                b.set_prompt(i, p)
            b.decode(12, use_graph)
            got[on] = [b.logits(i).astype(np.float64) for i in range(2)]
        for i in range(2):
            err = np.linalg.norm(got[1][i] - got[0][i]) / np.linalg.norm(got[0][i])
            print(f"{wdt} slot {i}: logits rel-L2 to option 0 = {err:.3e}")
            assert 0 < err < LOGIT_TOL, err  # (0: the option changed nothing)


@WDT
def test_option_off_again_is_the_default_path(wdt):
    """Captured steps of the option-on path must not survive the switch back."""
    prompts = [_prompt(5, 6), _prompt(6, 9)]
    with _batch(wdt, 2) as b:
        want = b.generate(prompts, N_NEW)
        want_l = [_bits(b.logits(i)) for i in range(2)]
        b.set_option("rows_mfma", 1)
        b.generate(prompts, N_NEW)
        b.set_option("rows_mfma", 0)
        got = b.generate(prompts, N_NEW)
        for i in range(2):
            assert np.array_equal(got[i], want[i])
            assert np.array_equal(_bits(b.logits(i)), want_l[i])
