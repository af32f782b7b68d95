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


# ---- where cutState comes from: the slot's plan (restir_amd/csrc/rs_cut_plan.h through rs_debug_plan_primary_cut_slot) ------------------
NOTHING, NO_MEMORY, BUILT = capi.CUT_ARENA_NOTHING, capi.CUT_ARENA_NO_MEMORY, capi.CUT_ARENA_BUILT


def _key(**changes):
    from restir_amd.ctypes_structs import make_camera
    cam = capi.camera_update(make_camera(96, 54, position=(0.1, 0.5, 1.2), rotation=(-80.0, -5.0, 0.0), fov_y=12.0))
    k = capi.PrimaryCutKey(sceneId=7, geomEdits=3, cam=cam, y0=0, y1=54, cap=4096, listCap=192)
    for name, value in changes.items():
        setattr(k, name, value)
    return k


def _call(slot, key, **kw):
    return capi.plan_primary_cut_slot(slot, key, **kw)[0]


def _built(slot, cuts=BUILT, lists=BUILT):
    """What the build leaves in the slot (primary_cuts.hip rs_primary_cuts_build)."""
    slot.cuts, slot.lists = cuts, lists


def _arenas(slot):
    return slot.keyValid, slot.cuts, slot.lists


@pytest.mark.parametrize("on,capturing", [(False, False), (True, True), (False, True)], ids=["off", "capturing", "off-capturing"])
def test_switch_off_or_capturing_forgets_both_arenas(on, capturing):
    for cuts, lists in ((NOTHING, NOTHING), (BUILT, BUILT), (BUILT, NO_MEMORY), (NO_MEMORY, NOTHING)):
        slot = capi.PrimaryCutSlot()
        assert _call(slot, _key()) == 0
        _built(slot, cuts, lists)
        assert _call(slot, _key(), on=on, capturing=capturing) == 0
        assert _arenas(slot) == (0, NOTHING, NOTHING)
        assert _call(slot, _key()) == 0 and _arenas(slot) == (1, NOTHING, NOTHING)         # the same key again: a first sight


def test_one_key_over_three_calls():
    slot = capi.PrimaryCutSlot()
    assert _call(slot, _key()) == 0 and _arenas(slot) == (1, NOTHING, NOTHING)
    assert _call(slot, _key()) == 1 and _arenas(slot) == (1, NOTHING, NOTHING)
    assert _call(slot, _key()) == 1                                 # until the build has run
    _built(slot)
    assert _call(slot, _key()) == 2 and _arenas(slot) == (1, BUILT, BUILT)
    assert _call(slot, _key()) == 2


def test_no_memory_for_the_cuts_stays_until_a_new_key():
    slot = capi.PrimaryCutSlot()
    _call(slot, _key())
    assert _call(slot, _key()) == 1
    _built(slot, NO_MEMORY, NOTHING)
    for _ in range(3):
        assert _call(slot, _key()) == 0 and _arenas(slot) == (1, NO_MEMORY, NOTHING)
    assert _call(slot, _key(geomEdits=4)) == 0 and _arenas(slot) == (1, NOTHING, NOTHING)
    assert _call(slot, _key(geomEdits=4)) == 1


def test_no_memory_for_the_lists_leaves_the_cuts():
    slot = capi.PrimaryCutSlot()
    _call(slot, _key())
    _built(slot, BUILT, NO_MEMORY)
    for _ in range(2):
        assert _call(slot, _key()) == 2 and _arenas(slot) == (1, BUILT, NO_MEMORY)
    assert _call(slot, _key(y1=46)) == 0 and _arenas(slot) == (1, NOTHING, NOTHING)


def _camera_byte(k, at):
    import ctypes as C
    b = (C.c_ubyte * C.sizeof(k.cam)).from_buffer(k.cam)
    b[at] ^= 1


KEY_CHANGES = dict(sceneId=dict(sceneId=8), geomEdits=dict(geomEdits=4), y0=dict(y0=8), y1=dict(y1=46), cap=dict(cap=4095), listCap=dict(listCap=0))


@pytest.mark.parametrize("member", list(KEY_CHANGES) + ["camera_first_byte", "camera_last_byte", "camera_middle_byte"])
def test_every_member_of_the_key_counts(member):
    import ctypes as C
    slot = capi.PrimaryCutSlot()
    _call(slot, _key())
    _built(slot)
    assert _call(slot, _key()) == 2
    if member in KEY_CHANGES:
        other = _key(**KEY_CHANGES[member])
    else:
        other = _key()
        _camera_byte(other, dict(camera_first_byte=0, camera_last_byte=C.sizeof(other.cam) - 1, camera_middle_byte=C.sizeof(other.cam) // 2)[member])
    assert _call(slot, other) == 0 and _arenas(slot) == (1, NOTHING, NOTHING), member
    assert _call(slot, other) == 1                                 # the new key is the stored one
    assert _call(slot, _key()) == 0                                 # and the old one is another key now


def _sizes(tiles, cap, list_cap):
    z = capi.plan_primary_cut_slot(capi.PrimaryCutSlot(), _key(cap=cap, listCap=list_cap), tiles=tiles)[1]
    return z.numCells, z.capacity, z.numTiles, z.listCapacity


def test_arena_sizes():
    """min(cap, 512) records per block, four tiles per block, min(listCap, 32) records per tile; listCap 0: no lists."""
    assert _sizes((1, 1), 1, 192) == (1, 1, 4, 128)
    assert _sizes((1, 1), 512, 192) == (1, 512, 4, 128)
    assert _sizes((1, 1), 513, 192) == (1, 512, 4, 128)
    assert _sizes((1, 1), 1 << 24, 192) == (1, 512, 4, 128)
    assert _sizes((60, 135), 4096, 192) == (8100, 8100 * 512, 32400, 32400 * 32)         # 1920 x 1080
    assert _sizes((3, 7), 8, 0) == (21, 168, 0, 0)
    assert _sizes((3, 7), 8, 32) == (21, 168, 84, 84 * 32)
    assert _sizes((3, 7), 8, 33) == (21, 168, 84, 84 * 32)
    assert _sizes((3, 7), 8, 5) == (21, 168, 84, 84 * 5)
    # the clamps: 2^22 blocks of 512 records are 2^31 > 0x7fffffff; 2^21 tiles of 32 records are 2^26 > 0x3ffffff
    assert _sizes((2048, 2048), 4096, 0) == (1 << 22, 0x7fffffff, 0, 0)
    assert _sizes((2048, 2047), 4096, 0) == (2048 * 2047, 2048 * 2047 * 512, 0, 0)
    assert _sizes((1024, 512), 1, 192) == (1 << 19, 1 << 19, 1 << 21, 0x3ffffff)
    assert _sizes((1024, 511), 1, 192) == (1024 * 511, 1024 * 511, 4096 * 511, 4096 * 511 * 32)
