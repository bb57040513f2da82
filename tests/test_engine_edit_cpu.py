"""CPU-side checks of the sequence-edit and draft-model entry points (no GPU needed): the built
library exports them with the documented argument types, the header declares them, and
Engine.generate keeps its old defaults."""
import ctypes as C
import inspect

import pytest

from llmi import _lib
from llmi.engine import Batch, Engine

_P, _I = C.c_void_p, C.c_int

DOCUMENTED = {
    # int llmi_engine_edit(llmi_engine* e, int keep, const int32_t* ids, int n)
    "llmi_engine_edit": [_P, _I, _P, _I],
    # int llmi_engine_position(llmi_engine* e, int* next_pos, int* prompt_len)
    "llmi_engine_position": [_P, C.POINTER(_I), C.POINTER(_I)],
    # int llmi_batch_edit(llmi_batch* b, int seq, int keep, const int32_t* ids, int n)
    "llmi_batch_edit": [_P, _I, _I, _P, _I],
    # int llmi_engine_generate_draft(target, draft, n_steps, max_draft, draft_prefill, use_graph, stats)
    "llmi_engine_generate_draft": [_P, _P, _I, _I, _I, _I, C.POINTER(_lib.SpecStats)],
}


@pytest.mark.parametrize("name", sorted(DOCUMENTED))
def test_symbol_is_exported_with_the_documented_argtypes(name):
    L = _lib.lib()
    assert name in _lib.header_functions()
    fn = getattr(L, name)
    assert fn.restype is _I
    assert list(fn.argtypes) == DOCUMENTED[name]


def test_null_handles_are_argument_errors():
    L = _lib.lib()
    assert L.llmi_engine_edit(None, 0, None, 0) == -1
    assert L.llmi_engine_position(None, None, None) == -1
    assert L.llmi_batch_edit(None, 0, 0, None, 0) == -1
    assert L.llmi_engine_generate_draft(None, None, 1, 1, 0, 1, None) == -1
    assert b"[llmi][ERROR]" in L.llmi_last_error()


def test_python_surface_and_generate_defaults():
    for name in ("edit", "position", "extend", "generate_draft"):
        assert callable(getattr(Engine, name))
    assert callable(Batch.edit)
    p = inspect.signature(Engine.generate).parameters
    assert list(p) == ["self", "prompt", "n_new", "use_graph", "prefill", "exact", "speculate", "ngram", "draft"]
    defaults = {k: v.default for k, v in p.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(use_graph=True, prefill=False, exact=True, speculate=0, ngram=(3, 1), draft=None)
    g = inspect.signature(Engine.generate_draft).parameters
    assert list(g) == ["self", "draft", "n_steps", "max_draft", "prefill", "use_graph"]
    assert g["prefill"].default is False and g["use_graph"].default is True
