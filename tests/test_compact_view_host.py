"""The compact views (include/pom_batch.h PomCompactViewSpec) without a GPU: the checker (tests/compact_view_oracle.py) on hand-made
states, every expectation written out; the kernel's byte mapping (pomcpp_amd/csrc/pom_observe_compact.h) built for the host
(tests/emul/pom_compact_view_emul.cpp) against the checker for every mask, radius and form at batch sizes with every pass length and
tail; that build as a stand-alone program under the host sanitizers; the struct's layout, its mirror and the wrapper's argument rules."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from pomcpp_amd import _abi
from pomcpp_amd.batch import BatchEnvironment, _CompactViewSpec, _MixedStepSpec, _ViewSpec
from tests import compact_view_oracle as co
from tests import host_build
from tests import view_oracle as vo
from tests import wrapper_standin as W
from tests.compact_view_cases import PLACES, hand_states
from tests.test_observe_view import _case, _ob
from tests.wrapper_standin import Duck

EMUL_SRC = "tests/emul/pom_compact_view_emul.cpp"
RADII = (0, 1, 4, 5, 10)
I32, U8, N = W.I32, W.U8, W.N


@pytest.fixture(scope="module")
def hand():
    """the hand-made states' unfogged arrays, computed once and shared (read only)"""
    ob = _ob()
    states = hand_states()
    _, attrs, env2 = ob.observe(states, per_agent=True)
    out = dict(states=states, attrs=attrs, env2=env2, codes=ob.observe_codes(states))
    for a in out.values():
        a.setflags(write=False)
    return out


def _views(case, radius):
    return vo.view_codes(case["codes"], case["attrs"], radius)


def test_the_hand_made_viewers_stand_where_they_should(hand):
    x, y, alive = hand["attrs"][:, :, 0], hand["attrs"][:, :, 1], hand["attrs"][:, :, 2]
    assert [[(int(x[e, a]), int(y[e, a]), int(not alive[e, a])) for a in range(4)] for e in range(3)] == PLACES
    spots = {p[:2] for places in PLACES for p in places}
    assert {(0, 0), (10, 0), (0, 10), (10, 10)} <= spots                      # the corners
    assert {(5, 0), (0, 5), (10, 5), (5, 10)} <= spots and (5, 5) in spots     # the edges, the middle
    assert sum(p[2] for places in PLACES for p in places) == 1                 # a dead viewer


def test_uncentred_is_row_selection(hand):
    for r in RADII:
        four = _views(hand, r)
        for mask in range(1, 16):
            got = co.compact_codes(four, hand["attrs"], r, mask, False)
            ids = co.viewers_of(mask)
            assert got.shape == (3, len(ids), 5, 11, 11) and got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
            for j, v in enumerate(ids):
                assert np.array_equal(got[:, j], four[:, v]), (r, mask, v)
            va = vo.viewer_attrs(hand["attrs"], hand["env2"][:, 0])
            assert np.array_equal(co.compact_viewer_attrs(va, mask), va[:, ids])
    assert co.viewers_of(0b0101) == [0, 2] and co.viewers_of(0b1110) == [1, 2, 3]


def test_a_corner_viewer_at_radius_4(hand):
    """the viewer at (0, 0): exactly the first four rows and columns of the 9 x 9 crop lie off the board"""
    crop = co.compact_codes(_views(hand, 4), hand["attrs"], 4, 0b0001, True)[0, 0]
    assert crop.shape == (5, 9, 9)
    off = np.zeros((9, 9), dtype=bool)
    off[:4, :] = off[:, :4] = True
    assert np.array_equal(crop[0] == 5, off)                                   # 5 in plane 0: off the board and nothing else
    assert (crop[1:, off] == 0).all()
    assert crop[0, 4, 4] == 10                                                 # the viewer in the middle of its crop
    assert np.array_equal(crop[:, 4:, 4:], hand["codes"][0][:, :5, :5])        # and the board's corner behind it, unfogged
    # the opposite corner (10, 10): the last four rows and columns
    crop = co.compact_codes(_views(hand, 4), hand["attrs"], 4, 0b1000, True)[0, 0]
    assert np.array_equal(crop[0] == 5, off[::-1, ::-1]) and crop[0, 4, 4] == 13
    assert np.array_equal(crop[:, :5, :5], hand["codes"][0][:, 6:, 6:])


def test_edges_the_middle_and_the_dead_viewer(hand):
    four = _views(hand, 4)
    edges = co.compact_codes(four, hand["attrs"], 4, 15, True)[1]             # (5, 0), (0, 5), (10, 5), (5, 10)
    fog = [(c[0] == 5) for c in edges]
    assert fog[0][:4].all() and not fog[0][4:].any()                           # the top edge: four rows off the board, no column
    assert fog[1][:, :4].all() and not fog[1][:, 4:].any()
    assert fog[2][:, 5:].all() and not fog[2][:, :5].any()
    assert fog[3][5:].all() and not fog[3][:5].any()
    mid = co.compact_codes(four, hand["attrs"], 4, 0b0001, True)[2, 0]         # (5, 5): nothing off the board
    assert not (mid[0] == 5).any() and np.array_equal(mid, hand["codes"][2][:, 1:10, 1:10])
    assert (mid[0, 4, 6], mid[1, 4, 6], mid[2, 4, 6]) == (3, 3, 6)             # the bomb at (7, 5): code, strength, life
    assert (mid[0, 2, 4], mid[4, 2, 4]) == (4, 2)                              # the flame at (5, 3) and its life
    dead = co.compact_codes(four, hand["attrs"], 4, 0b0100, True)[2, 0]        # looks out from (10, 3), where it died
    off = np.repeat(np.arange(9)[None] > 4, 9, axis=0)                         # x 11..14, and the row y = -1
    off[0] = True
    assert np.array_equal(dead[0] == 5, off)
    assert np.array_equal(dead[:, 1:, :5], hand["codes"][2][:, :8, 6:]) and dead[0, 4, 4] == 0
    va = co.compact_viewer_attrs(vo.viewer_attrs(hand["attrs"], hand["env2"][:, 0]), 0b0100)
    assert va.shape == (3, 1, 12) and va[2, 0, :3].tolist() == [10, 3, 0] and va[2, 0, 11] == 19


def test_radius_0_and_radius_10(hand):
    """r = 0: the viewer's own cell; r = 10: the 21 x 21 crop holds the board exactly once"""
    one = co.compact_codes(_views(hand, 0), hand["attrs"], 0, 15, True)
    assert one.shape == (3, 4, 5, 1, 1)
    for e in range(3):
        for v, (x, y, _) in enumerate(PLACES[e]):
            assert np.array_equal(one[e, v, :, 0, 0], hand["codes"][e][:, y, x])
    big = co.compact_codes(_views(hand, 10), hand["attrs"], 10, 15, True)
    assert big.shape == (3, 4, 5, 21, 21)
    for e in range(3):
        for v, (x, y, _) in enumerate(PLACES[e]):
            on = np.zeros((21, 21), dtype=bool)
            on[10 - y:21 - y, 10 - x:21 - x] = True
            assert np.array_equal(big[e, v][:, on].reshape(5, 11, 11), hand["codes"][e])
            assert (big[e, v, 0][~on] == 5).all() and (big[e, v, 1:][:, ~on] == 0).all()
    for r in (1, 5):
        assert co.compact_codes(_views(hand, r), hand["attrs"], r, 0b0110, True).shape == (3, 2, 5, 2 * r + 1, 2 * r + 1)


# ---- the kernel's byte mapping, built for the host --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    lib = C.CDLL(host_build.shared_lib(EMUL_SRC))
    lib.pom_emul_compact_views.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pom_emul_compact_views.restype = C.c_int64
    lib.pom_emul_compact_rank.argtypes = [C.c_int32] * 3

    def views(codes, attrs, radius, mask, centred, guard=32):
        """(the array, the guard bytes before and after it still 0xAB)"""
        n, k, s = len(codes), bin(mask).count("1"), co.side(radius, centred)
        size = n * k * 5 * s * s
        buf = np.full(size + 2 * guard, 0xAB, dtype=np.uint8)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        xy = np.ascontiguousarray(attrs[:, :, 0] | (attrs[:, :, 1] << 4), dtype=np.uint8)
        wrote = lib.pom_emul_compact_views(n, mask, int(centred), radius, codes.ctypes.data, xy.ctypes.data, buf.ctypes.data + guard)
        assert wrote == size
        return buf[guard:guard + size].reshape(n, k, 5, s, s), bool((buf[:guard] == 0xAB).all() and (buf[guard + size:] == 0xAB).all())
    return views, lib


@pytest.fixture(scope="module")
def batch(hand):
    """17 envs: the three hand-made ones, then mid-game stress games — unfogged codes and agent_attrs, read only"""
    game = _case("stress", 16, 23)
    codes = np.concatenate([hand["codes"], game["codes"][:14]])
    attrs = np.concatenate([hand["attrs"], game["attrs"][:14]])
    codes.setflags(write=False)
    attrs.setflags(write=False)
    return codes, attrs


def test_the_byte_mapping_equals_the_checker(emul, batch):
    """all 15 masks x 11 radii x both forms, at n = 1, 2, 3, 4, 5, 17: every pass length, and every tail a short pass can end with"""
    views, _ = emul
    codes, attrs = batch
    tails = set()
    for r in range(11):
        four = vo.view_codes(codes, attrs, r)                                  # once per radius, for the 17
        for centred in (False, True):
            for mask in range(1, 16):
                want = co.compact_codes(four, attrs, r, mask, centred)
                for n in (1, 2, 3, 4, 5, 17):
                    got, guards = views(codes[:n], attrs[:n], r, mask, centred)
                    assert guards, (r, centred, mask, n)
                    assert np.array_equal(got, want[:n]), (r, centred, mask, n)
                    tails.add((n % 4) * int(np.prod(want.shape[1:])) % 4)
    assert tails == {0, 1, 2, 3}


def test_viewer_attrs_rows(emul):
    _, lib = emul
    for mask in range(1, 16):
        ids = co.viewers_of(mask)
        for centred in (0, 1):
            assert [lib.pom_emul_compact_rank(mask, centred, v) for v in range(4)] == [ids.index(v) if v in ids else -1 for v in range(4)]


def test_the_byte_mapping_under_the_host_sanitizers():
    """the stand-alone program: the same sweep between guard bytes in exactly-sized heap blocks, under ASan and UBSan"""
    exe = host_build.program(EMUL_SRC, name="pom_compact_view_emul_asan", extra=["-DPOM_COMPACT_VIEW_EMUL_MAIN"], sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout + r.stderr


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_structs_layout(tmp_path):
    """size 56, the offsets 40 / 44 / 48, the PomViewSpec first — as gcc sees the header; and the mirror"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pom_batch.h"\n'
                   '_Static_assert(sizeof(PomCompactViewSpec) == POM_COMPACT_VIEW_SPEC_SIZE, "size");\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(PomCompactViewSpec), offsetof(PomCompactViewSpec, view),\n'
                   '  offsetof(PomCompactViewSpec, viewer_mask), offsetof(PomCompactViewSpec, flags), offsetof(PomCompactViewSpec, reserved2_),\n'
                   '  (int)POM_VIEW_CENTRED, (int)POM_VIEW_SPEC_SIZE); return 0; }\n')
    exe = host_build.program(str(src))
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["56", "0", "40", "44", "48", "1", "40"]
    assert C.sizeof(_CompactViewSpec) == 56 and _abi.VIEW_CENTRED == 1
    assert [(f, getattr(_CompactViewSpec, f).offset, getattr(_CompactViewSpec, f).size) for f, _ in _CompactViewSpec._fields_] == \
        [("view", 0, 40), ("viewer_mask", 40, 4), ("flags", 44, 4), ("reserved2_", 48, 8)]
    assert _CompactViewSpec._fields_[0][1] is _ViewSpec
    head = _abi._view_spec(3, 4, 0x1000, 0x2000, 0x3000, compact=(0b0101, 1))
    assert isinstance(head, _ViewSpec) and (head.struct_size, head.dtype, head.view_radius, head.reserved_) == (56, 3, 4, 0)
    whole = C.cast(C.pointer(head), C.POINTER(_CompactViewSpec)).contents
    assert (whole.viewer_mask, whole.flags, whole.reserved2_, whole.view.planes_dev, whole.view.env_attrs_dev) == (5, 1, 0, 0x1000, 0x3000)
    assert _abi._view_spec(3, 4, 0x1000).struct_size == 40


# ---- the wrapper's argument rules -------------------------------------------------------------------------------------------------
def _compact_of(view_pointer):
    return C.cast(view_pointer, C.POINTER(_CompactViewSpec)).contents


def test_the_wrapper_builds_the_compact_spec():
    env = W.handle(BatchEnvironment)
    mv, ev = Duck((N, 4), I32), Duck((N, 4), I32)
    for viewers, centred, r, k, s, mask in (([0], True, 4, 1, 9, 1), (0b0101, False, 4, 2, 11, 5), ((3, 1, 2), True, 0, 3, 1, 14),
                                            (None, True, 10, 4, 21, 15), (15, False, 2, 4, 11, 15)):
        codes, va, ea = Duck((N, k, 5, s, s), U8), Duck((N, k, 12), I32), Duck((N, 4), I32)
        kw = dict(codes=codes, view_radius=r, viewer_attrs=va, env_attrs=ea, viewers=viewers, centred=centred)
        env.step_mixed(0, 16, mv, 0b1110, 9, 3, **kw)
        env.step_events(16, 4, mv, 0b1110, 9, 3, ev, **kw)
        for (entry, args), want in zip(env._lib.calls, ("pom_batch_step_mixed", "pom_batch_step_events")):
            assert entry == want
            step = args[1]._obj
            assert isinstance(step, _MixedStepSpec) and step.simple_mask == 0b1110 and not step.planes_dev
            c = _compact_of(step.view)
            assert (c.view.struct_size, c.view.dtype, c.view.view_radius, c.view.reserved_) == (56, 3, r, 0)
            assert (c.viewer_mask, c.flags, c.reserved2_) == (mask, int(centred), 0)
            assert (c.view.planes_dev, c.view.viewer_attrs_dev, c.view.env_attrs_dev) == (codes.address, va.address, ea.address)
        env._lib.calls.clear()
    # the defaults are today's spec
    env.step_mixed(0, 16, mv, 0, 9, 3, codes=Duck((N, 4, 5, 11, 11), U8), view_radius=4, viewer_attrs=Duck((N, 4, 12), I32))
    assert env._lib.calls.pop()[1][1]._obj.view.contents.struct_size == 40


def test_the_wrapper_refuses_before_any_call():
    env = W.handle(BatchEnvironment)
    mv, ev = Duck((N, 4), I32), Duck((N, 4), I32)
    good = dict(codes=Duck((N, 1, 5, 9, 9), U8), view_radius=4, viewer_attrs=Duck((N, 1, 12), I32), viewers=[0], centred=True)
    bad = {
        "the four-view shape": dict(good, codes=Duck((N, 4, 5, 11, 11), U8)),
        "uncropped": dict(good, codes=Duck((N, 1, 5, 11, 11), U8)),
        "one viewer too many": dict(good, codes=Duck((N, 2, 5, 9, 9), U8)),
        "the radius' side": dict(good, view_radius=3),
        "int8": dict(good, codes=Duck((N, 1, 5, 9, 9), W.I8)),
        "a strided slice": dict(good, codes=Duck((N, 1, 5, 9, 9), U8, contiguous=False)),
        "viewer_attrs of four": dict(good, viewer_attrs=Duck((N, 4, 12), I32)),
        "no viewer": dict(good, viewers=[]),
        "mask 0": dict(good, viewers=0),
        "mask 16": dict(good, viewers=16),
        "agent 4": dict(good, viewers=[4]),
        "planes": dict({k: v for k, v in good.items() if k != "codes"}, planes=Duck((N, 1, 16, 9, 9), U8)),
        "no radius": dict(good, view_radius=None),
        "uncentred with the crop's shape": dict(good, centred=False),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            env.step_mixed(0, 16, mv, 0b1110, 9, 3, **kw)
        with pytest.raises(ValueError):
            env.step_events(0, 16, mv, 0b1110, 9, 3, ev, **kw)
        assert not env._lib.calls, what
    env.step_mixed(0, 16, mv, 0b1110, 9, 3, **good)
    assert len(env._lib.calls) == 1


def test_observe_allocates_the_compact_shapes(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = W.handle(BatchEnvironment)
    planes, va, ea = env.observe(dtype="codes", view_radius=4, viewers=[0, 3], centred=True)
    assert planes.shape == (N, 2, 5, 9, 9) and planes.dtype == U8 and va.shape == (N, 2, 12) and ea.shape == (N, 4)
    (entry, args), = env._lib.calls
    assert entry == "pom_batch_observe_view"
    c = _compact_of(C.pointer(args[1]._obj))
    assert (c.view.struct_size, c.viewer_mask, c.flags, c.view.planes_dev, c.view.viewer_attrs_dev) == (56, 9, 1, planes.address, va.address)
    env._lib.calls.clear()
    planes, va, _ = env.observe(dtype="codes", view_radius=2, viewers=0b0100)
    assert planes.shape == (N, 1, 5, 11, 11) and va.shape == (N, 1, 12)
    env._lib.calls.clear()
    for kw in (dict(dtype="uint8", view_radius=4, viewers=[0]), dict(dtype="codes", viewers=[0]), dict(dtype="codes", view_radius=4, viewers=[]),
               dict(dtype="codes", view_radius=4, centred=True, out=Duck((N, 4, 5, 11, 11), U8))):
        with pytest.raises(ValueError):
            env.observe(**kw)
    with pytest.raises(ValueError):
        env.observe(dtype="codes", view_radius=4, viewers=[0], _step_moves=Duck((N, 4), I32))   # (step_device_observe()'s way in)
    assert not env._lib.calls
    planes, va, _ = env.observe(dtype="codes", view_radius=4)             # the defaults: today's four views
    assert planes.shape == (N, 4, 5, 11, 11) and va.shape == (N, 4, 12) and env._lib.calls[0][1][1]._obj.struct_size == 40
