"""CPU: the host side of tests/perturb.py - the wrappers go onto the instance and come off again, in order and also when the
wrapped walk raises; the list of stream-taking entry points matches the parsed C ABI."""
import ctypes

import pytest

from tests import perturb


class _Walk:
    """the four methods perturb wraps, recording the order they ran in"""

    def __init__(self):
        self.log = []

    def _fork(self):
        self.log.append("fork")
        return "streams"

    def _join(self):
        self.log.append("join")

    def _wg_launch(self, fn, keep):
        self.log.append("launch")
        fn()

    def _wg_join(self):
        self.log.append("wg_join")


def test_wrappers_sit_on_the_instance_and_are_removed():
    m = _Walk()
    with perturb.timed(m) as t:
        assert all(n in m.__dict__ for n in perturb._Wrapped.NAMES)
        assert m._fork() == "streams"          # the wrapped method's result passes through
        m._wg_launch(lambda: m.log.append("fn"), ())
        m._join()
        m._wg_join()
        with pytest.raises(AssertionError):    # one set of wrappers at a time
            perturb.timed(m).__enter__()
    assert m.log == ["fork", "launch", "fn", "join", "wg_join"]
    assert t.sections == 1 and t.longest > 0.0
    assert not any(n in m.__dict__ for n in perturb._Wrapped.NAMES)
    assert m._fork.__func__ is _Walk._fork


def test_wrappers_are_removed_when_the_walk_raises():
    m = _Walk()
    with pytest.raises(ZeroDivisionError):
        with perturb.timed(m):
            m._fork()
            1 / 0
    assert not any(n in m.__dict__ for n in perturb._Wrapped.NAMES)


def test_delayed_refuses_what_the_sleeper_refuses():
    m = _Walk()
    for which, micros in (("trunk3", 10), ("main", 0), ("main", perturb.MAX_MICROS + 1)):
        with pytest.raises(AssertionError):
            perturb.delayed(m, which, micros)


def test_stream_entry_points_match_the_parsed_abi():
    from deepsense6g_tii_amd import _lib
    protos = _lib.parse_header()
    names = perturb.stream_entry_points()
    assert len(names) == len(set(names)) > 100 and "debug_occupy_cus" in names
    for n in names:
        assert protos["ds6g_" + n][1][-1] is ctypes.c_void_p, n
    # the entry points that end in a pointer which is no stream: the three planners and the salt pointer
    rest = {k for k, (_, a) in protos.items() if a and a[-1] is ctypes.c_void_p} - {"ds6g_" + n for n in names}
    assert rest == {"ds6g_gemm_plan", "ds6g_attention_plan", "ds6g_winograd_plan", "ds6g_set_dropout_salt"}, rest
