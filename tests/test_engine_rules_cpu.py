"""CPU-side checks of the logit-rules entry points of Engine and Batch (no GPU needed): the built
library exports them with the documented argument types, the header declares them, null handles
are argument errors, the Python methods have the documented signatures, Engine.generate keeps
its signature, and Engine.choose validates its choices before it touches an engine."""
import ctypes as C
import inspect

import pytest

from llmi import _lib
from llmi.engine import Batch, Engine, choice_trie

_P, _I, _F = C.c_void_p, C.c_int, C.c_float

DOCUMENTED = {
    # int llmi_engine_set_logit_rules(e, const int32_t* bias_ids, const float* bias_values, int n_bias,
    #                                 float presence_penalty, float frequency_penalty, int count_prompt)
    "llmi_engine_set_logit_rules": [_P, _P, _P, _I, _F, _F, _I],
    # int llmi_engine_set_allowed(e, const int32_t* ids, int n)
    "llmi_engine_set_allowed": [_P, _P, _I],
    # int llmi_engine_clear_logit_rules(e)
    "llmi_engine_clear_logit_rules": [_P],
    # int llmi_engine_processed_logits(e, float* out, int n)
    "llmi_engine_processed_logits": [_P, _P, _I],
    # the batch forms: the same with a seq argument after the handle
    "llmi_batch_set_logit_rules": [_P, _I, _P, _P, _I, _F, _F, _I],
    "llmi_batch_set_allowed": [_P, _I, _P, _I],
    "llmi_batch_clear_logit_rules": [_P, _I],
    "llmi_batch_processed_logits": [_P, _I, _P, _I],
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
    for rc in (L.llmi_engine_set_logit_rules(None, None, None, 0, 0.0, 0.0, 0),
               L.llmi_engine_set_allowed(None, None, 0),
               L.llmi_engine_clear_logit_rules(None),
               L.llmi_engine_processed_logits(None, None, 0),
               L.llmi_batch_set_logit_rules(None, 0, None, None, 0, 0.0, 0.0, 0),
               L.llmi_batch_set_allowed(None, 0, None, 0),
               L.llmi_batch_clear_logit_rules(None, 0),
               L.llmi_batch_processed_logits(None, 0, None, 0)):
        assert rc == -1
        assert b"[llmi][ERROR]" in L.llmi_last_error()


def _params(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items()}


def test_python_surface():
    E = inspect.Parameter.empty
    assert _params(Engine.set_logit_rules) == dict(self=E, bias=None, presence_penalty=0.0, frequency_penalty=0.0,
                                                   count_prompt=False)
    assert list(_params(Engine.set_allowed)) == ["self", "ids"]
    assert list(_params(Engine.clear_logit_rules)) == ["self"]
    assert list(_params(Engine.processed_logits)) == ["self"]
    assert _params(Engine.choose) == dict(self=E, prompt=E, choices=E, use_graph=True)
    assert _params(Batch.set_logit_rules) == dict(self=E, seq=E, bias=None, presence_penalty=0.0,
                                                  frequency_penalty=0.0, count_prompt=False)
    assert list(_params(Batch.set_allowed)) == ["self", "seq", "ids"]
    assert list(_params(Batch.clear_logit_rules)) == ["self", "seq"]
    assert list(_params(Batch.processed_logits)) == ["self", "seq"]


def test_generate_keeps_its_signature():
    p = inspect.signature(Engine.generate).parameters
    assert list(p) == ["self", "prompt", "n_new", "use_graph", "prefill", "exact", "speculate", "ngram", "draft"]
    defaults = {k: v.default for k, v in p.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(use_graph=True, prefill=False, exact=True, speculate=0, ngram=(3, 1), draft=None)


@pytest.mark.parametrize("choices", [
    [],                      # no choice
    [[1, 2], []],            # an empty choice
    [[1, 2], [3], [1, 2]],   # duplicates
    [[1, 2, 3], [1, 2]],     # a choice that is a prefix of another (the longer one first)
    [[1, 2], [1, 2, 3]],     # ... and the shorter one first
])
def test_choose_validates_its_choices_before_it_touches_an_engine(choices):
    no_engine = object.__new__(Engine)  # no handle, no attribute: any use of it would raise AttributeError
    with pytest.raises(ValueError):
        Engine.choose(no_engine, [1, 2, 3], choices)
    with pytest.raises(ValueError):
        choice_trie(choices)


def test_choice_trie_of_valid_choices():
    nodes = choice_trie([[5], [7, 1], [7, 2, 9]])
    assert sorted(nodes[0]["next"]) == [5, 7]
    assert nodes[nodes[0]["next"][5]]["leaf"] == 0
    seven = nodes[nodes[0]["next"][7]]
    assert seven["leaf"] == -1 and sorted(seven["next"]) == [1, 2]
    assert nodes[seven["next"][1]]["leaf"] == 1
    assert nodes[nodes[seven["next"][2]]["next"][9]]["leaf"] == 2
