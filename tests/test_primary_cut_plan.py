"""CPU: the primary-cut field of a phase-A plan (restir_amd/csrc/rs_frame_plan.h, rs_cuts.h), asked through rs_debug_phase_a_plan over
the forms of DESIGN.md section 4.  cutState is the caller's comparison of this call's key (scene geometry, camera, size, rows) with the
previous frame's: 0 off or another key, 1 unchanged and nothing built, 2 unchanged and built.  The plan's `cut` follows it wherever the
launch is k_primary / k_primary_split, is 0 in the fused launch and for an empty row range, and leaves every other field alone."""
import pytest

from restir_amd import capi
from tests.test_frame_plan import DEFAULTS, DENOISE, FULL, REUSED, STRIP, plan

OTHER_FIELDS = [n for n, _ in capi.PhaseAPlan._fields_ if n != "cut"]


def others(p):
    return tuple(getattr(p, n) for n in OTHER_FIELDS)


def test_the_default_input_changes_nothing():
    assert "cutState" not in DEFAULTS
    for groups in ((), (REUSED,), (STRIP,), (STRIP, REUSED), (DENOISE,), (dict(async_=0),), (REUSED, dict(idle=1))):
        base = plan(*groups)
        assert base.cut == 0
        for state in (1, 2):
            assert others(plan(*groups, cutState=state)) == others(base), (groups, state)


@pytest.mark.parametrize("geometry", [FULL, STRIP], ids=["full", "strip"])
@pytest.mark.parametrize("state", [0, 1, 2])
def test_a_reused_frame_follows_the_key(geometry, state):
    """A frame answered from retained G-buffer planes has no render to fuse: valid key and built -> the cuts; valid key, nothing built ->
    the build; another key or the switch off (both state 0) -> the tree.  The same on every chain, for the frame's later calls, with one
    frame at a time, with a denoise stream and in synchronous mode."""
    for extra in (dict(), dict(chain=1, smallChain=2), dict(phaseACalls=1), dict(phaseACalls=2), dict(idle=1), DENOISE, dict(async_=0)):
        p = plan(geometry, REUSED, extra, cutState=state)
        assert p.fuse == 0 and p.cut == state, (extra, state)


@pytest.mark.parametrize("state", [1, 2])
def test_the_fused_launch_keeps_the_tree(state):
    """A deferred render that rides in the primary rays' launch (a strip; a full frame inside the fused span or decided that way) walks
    two rays per pixel from 8x4 tiles: no cut is used or built there.  Two launches of the same frame take the cut."""
    assert plan(STRIP, cutState=state).fuse == 1 and plan(STRIP, cutState=state).cut == 0
    assert plan(FULL, tuneChoice=1, cutState=state).fuse == 1 and plan(FULL, tuneChoice=1, cutState=state).cut == 0
    assert plan(FULL, tuneFrame=20, cutState=state).cut == 0
    assert plan(FULL, tuneChoice=0, cutState=state).fuse == 0 and plan(FULL, tuneChoice=0, cutState=state).cut == state
    assert plan(STRIP, phaseACalls=1, cutState=state).cut == state          # the frame's second call is never fused


def test_no_rows_no_cut():
    assert plan(REUSED, y0=40, y1=40, cutState=2).cut == 0
    assert plan(REUSED, y0=40, y1=30, cutState=1).cut == 0
