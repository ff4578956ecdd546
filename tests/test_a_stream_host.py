"""nnlm_debug_set_a_stream (cache policy of the stream of A in the A-streaming cross products), host side -- no GPU: the export, the values
the hook accepts and the key nnlm_get_info answers.  What the policy does to results is tests/test_gpu_a_stream.py's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nnlm_amd import _lib  # noqa: E402

ERR_ARG = 1


def test_export_is_declared_and_listed():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    lib = _lib.load()
    name = "nnlm_debug_set_a_stream"
    assert name in _lib.EXPORTS and ("int " + name + "(int nt_from_stage);") in hdr and hasattr(lib, name)
    assert getattr(lib, name).argtypes == lib.nnlm_debug_set_xprod_waves.argtypes
    assert callable(_lib.debug_set_a_stream) and _lib.A_STREAM_NONE == 2**31 - 1


def test_hook_accepts_minus_one_and_every_stage_and_refuses_less():
    try:
        for v in (-1, 0, 1, 8, _lib.A_STREAM_NONE):
            _lib.debug_set_a_stream(v)
        for v in (-2, -(2**31)):
            with pytest.raises(_lib.NnlmError) as ei:
                _lib.debug_set_a_stream(v)
            assert ei.value.code == ERR_ARG and "nnlm_debug_set_a_stream" in str(ei.value)
    finally:
        _lib.debug_set_a_stream(-1)


def test_get_info_names_the_key():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    src = open(os.path.join(ROOT, "nnlm_amd", "csrc", "nnlm_mi355x.hip")).read()
    assert '"a_stream_nt_from"' in hdr
    assert 'strcmp(key, "a_stream_nt_from") == 0' in src
    assert "a_stream_nt_from" in _lib.Handle.get_info.__doc__
