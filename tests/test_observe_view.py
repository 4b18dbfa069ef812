"""Per-agent fogged views (pom_batch.h PomViewSpec): pom_batch_observe_view and its fused / range twins against
tests/view_oracle.py, which masks the UNFOGGED outputs of oracle/pom_observe_oracle.py by each viewer's window — bit-exact.
The states are played on the CPU (tests/oracle_lib.py) and uploaded, so what the fog has to hide is known before the GPU runs."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.state import Item, new_states
from tests import view_oracle as vo
from tests.host_build import ROOT, header_constant

KINDS = [("ffa", 0), ("ffa", 57), ("stress", 23)]
SIZES = [5, 16, 67, 200, 1001]
RADII = [0, 1, 4, 10]


@functools.lru_cache(maxsize=None)
def _ob():
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# Board seeds per (kind, batch size), picked on the CPU (tests/oracle_lib.py play) so that EVERY batch of a played kind tests fog at
# radius 4 (_fog_is_tested: each kind of thing on both sides of some window, a dead viewer, a window clipped on two sides).  Small
# batches hold that for few seeds only: 16 stress envs after 23 ticks rarely have an enemy within four cells.
SEEDS = {("ffa", 5): 5, ("ffa", 16): 3, ("ffa", 67): 3, ("ffa", 200): 3, ("ffa", 1001): 3,
         ("stress", 5): 3, ("stress", 16): 8, ("stress", 67): 5, ("stress", 200): 3, ("stress", 1001): 3}


@functools.lru_cache(maxsize=None)
def _case(kind, n, ticks, seed=None):
    """states played on the CPU and their unfogged observations, computed once and shared (nobody writes to them)"""
    from tests.oracle_lib import Oracle
    seed = SEEDS.get((kind, n), 3) if seed is None else seed
    start = pa.make_boards(n, seed=seed, kind=kind)
    states = start.copy()
    if ticks:
        Oracle().run_random(states, start, ticks, seed, 0, 0, 2 if kind == "stress" else 1, 300)
    states["agents"]["pad"] = 0
    ob = _ob()
    planes, attrs, env2 = ob.observe(states, per_agent=True)
    out = dict(states=states, planes=planes, attrs=attrs, env2=env2, codes=ob.observe_codes(states))
    for a in out.values():
        a.setflags(write=False)
    return out


def _env(states, **kw):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    env = BatchEnvironment(len(states), mode=MODE_ENV, **kw)
    env.make_game(states)
    return env


def _fog_is_tested(case, radius):
    """what the fog hides and what it shows, over the batch, read off the oracle's arrays: every kind of thing on both sides of
    some window, a dead viewer, a window clipped on two sides"""
    codes, attrs = case["codes"], case["attrs"]
    w = vo.windows(attrs, radius)                                      # [n, 4, 11, 11]
    board = np.broadcast_to(codes[:, None, 0], w.shape)
    viewer = 10 + np.arange(4)[None, :, None, None]
    kinds = {"bomb": board == 3, "flame": board == 4, "wood": board == 2, "power-up": (board >= 6) & (board <= 8),
             "enemy": (board >= 10) & (board <= 13) & (board != viewer)}
    for name, m in kinds.items():
        assert (m & ~w).any(), f"no {name} outside any window"
        assert (m & w).any(), f"no {name} inside any window"
    assert (attrs[:, :, 2] == 0).any(), "no dead viewer"
    x, y = attrs[:, :, 0], attrs[:, :, 1]
    clipped = ((x < radius) | (x > 10 - radius)) & ((y < radius) | (y > 10 - radius))
    assert clipped.any(), "no window clipped on two sides"


def test_view_oracle_on_a_hand_made_state():
    """a viewer in a corner, one at (5, 5), a dead one, and a bomb and a flame just inside and just outside the radius-2 window of
    the one at (5, 5); every expectation written out by hand"""
    ob = _ob()
    s = new_states(1)
    b = s["board"][0]                                                  # [y][x]
    for i, (x, y, dead) in enumerate([(0, 0, 0), (5, 5, 0), (10, 3, 1), (8, 9, 0)]):
        s["agents"][0, i]["x"], s["agents"][0, i]["y"], s["agents"][0, i]["dead"] = x, y, dead
        if not dead:
            b[y, x] = Item.AGENT0 + i
    s["aliveAgents"][0] = 3
    s["timeStep"][0] = 41
    b[5, 7] = Item.BOMB                                                # x = 7: |7 - 5| = 2, inside
    b[5, 8] = Item.BOMB                                                # x = 8: outside
    s["bombs_queue"][0, 0] = 7 + (5 << 4) + (1 << 8) + (3 << 12) + (6 << 16)
    s["bombs_queue"][0, 1] = 8 + (5 << 4) + (3 << 8) + (4 << 12) + (9 << 16)
    s["bombs_count"][0] = 2
    s["agents"][0, 1]["bombCount"] = 1
    s["agents"][0, 1]["maxBombCount"] = 2
    b[3, 5] = Item.FLAMES + ((5 + 11 * 3) << 3)                        # y = 3: inside
    b[2, 5] = Item.FLAMES + ((5 + 11 * 3) << 3)                        # y = 2: outside
    s["flames_queue"][0, 0]["x"], s["flames_queue"][0, 0]["y"], s["flames_queue"][0, 0]["timeLeft"] = 5, 3, 2
    s["flames_count"][0] = 1
    planes, attrs, env2 = ob.observe(s, per_agent=True)
    codes = ob.observe_codes(s)

    w = vo.windows(attrs, 2)
    assert w.shape == (1, 4, 11, 11)
    assert [int(w[0, v].sum()) for v in range(4)] == [9, 25, 15, 20]   # the corner, the middle, x 8..10 x y 1..5, x 6..10 x y 7..10
    assert w[0, 0, :3, :3].all() and w[0, 1, 3:8, 3:8].all() and w[0, 2, 1:6, 8:].all() and w[0, 3, 7:, 6:].all()

    c = vo.view_codes(codes, attrs, 2)
    assert c.shape == (1, 4, 5, 11, 11) and c.dtype == np.uint8
    assert c[0, 0, 0, 0, 0] == 10 and (c[0, 0, 0] == 5).sum() == 121 - 9 and (c[0, 0, 1:] == 0).all()
    assert (c[0, 1, 0, 5, 7], c[0, 1, 1, 5, 7], c[0, 1, 2, 5, 7]) == (3, 3, 6)      # the bomb inside: code, strength, life
    assert (c[0, 1, 0, 5, 8], c[0, 1, 1, 5, 8], c[0, 1, 2, 5, 8]) == (5, 0, 0)      # the bomb outside: fog, nothing
    assert (c[0, 1, 0, 3, 5], c[0, 1, 4, 3, 5]) == (4, 2) and (c[0, 1, 0, 2, 5], c[0, 1, 4, 2, 5]) == (5, 0)
    assert c[0, 1, 0, 5, 5] == 11 and c[0, 1, 0, 0, 0] == 5                         # itself by its absolute code; agent 0 in the fog
    assert (c[0, 2, 0, 5, 8], c[0, 2, 1, 5, 8]) == (3, 4) and c[0, 2, 0, 5, 7] == 5  # the dead viewer looks out from (10, 3)
    assert c[0, 3, 0, 9, 8] == 13 and (c[0, 3, 0] != 5).sum() == 20
    assert np.array_equal(vo.view_codes(codes, attrs, 10), np.repeat(codes[:, None], 4, axis=1))

    p = vo.view_planes(planes, attrs, 2)
    assert p.shape == (1, 4, 16, 11, 11)
    assert p[0, 0, 8, 0, 0] == 1 and p[0, 1, 8, 5, 5] == 1 and p[0, 3, 8, 9, 8] == 1  # plane 8: the viewer
    assert planes[0, 1, 11, 0, 0] == 1 and p[0, 1, :, 0, 0].sum() == 0              # agent 0 (plane 11 of view 1): fogged, all 16 zero
    assert (p[0, 1, 3, 5, 7], p[0, 1, 12, 5, 7], p[0, 1, 13, 5, 7]) == (1, 3, 6) and p[0, 1, :, 5, 8].sum() == 0
    assert (p[0, 1, 4, 3, 5], p[0, 1, 15, 3, 5]) == (1, 2) and p[0, 1, :, 2, 5].sum() == 0
    assert p[0, 1, :12].sum() == 25 and p[0, 2, :12].sum() == 15                    # one-hot inside, nothing outside
    assert np.array_equal(vo.view_planes(planes, attrs, 10), planes)

    va = vo.viewer_attrs(attrs, env2[:, 0])
    assert va.shape == (1, 4, 12) and va.dtype == np.int32
    assert va[0, 1].tolist() == [5, 5, 1, 1, 1, 2, 1, 0, 0, 1, 1, 41]               # alive flags of agents 2, 3, 0
    assert va[0, 2].tolist() == [10, 3, 0, 1, 0, 1, 1, 0, 1, 1, 1, 41]
    assert va[0, 3, 8:11].tolist() == [1, 1, 0]


def test_symbols_and_spec_size(hip_lib):
    """the three entry points are exported, and PomViewSpec is the size the header states (and the wrapper's structure has)"""
    from pomcpp_amd.batch import _ViewSpec
    for name in ("pom_batch_observe_view", "pom_batch_step_device_observe_view", "pom_batch_step_device_range_view"):
        assert hasattr(hip_lib, name), name
    assert header_constant("POM_VIEW_SPEC_SIZE") == C.sizeof(_ViewSpec) == 40
    assert header_constant("POM_OBS_VIEWER_ATTRS") == 12
    assert _ViewSpec.planes_dev.offset == 16 and _ViewSpec.viewer_attrs_dev.offset == 24 and _ViewSpec.env_attrs_dev.offset == 32


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_code_views_match_the_oracle(hip_lib, kind, ticks, n):
    """every radius, the array 0 / 4 / 8 bytes into a 16-byte line inside a larger buffer of 0xAB whose other bytes stay
    untouched; batch sizes with every remainder mod 4 and mod 16 and a last tile of fewer than four envs; attributes too"""
    import torch
    case = _case(kind, n, ticks)
    if ticks:   # (a start board has no bomb and no flame to hide)
        _fog_is_tested(case, 4)
        if n == 1001:
            _fog_is_tested(case, 1)
    size = n * 4 * 605
    with _env(case["states"]) as env:
        assert env.get_state().tobytes() == case["states"].tobytes()
        st = env.status()
        for radius in RADII:
            want = vo.view_codes(case["codes"], case["attrs"], radius)
            for off in (0, 4, 8):
                buf = torch.full((16 + size + 64,), 0xAB, dtype=torch.uint8, device="cuda")
                assert buf.data_ptr() % 16 == 0
                out = buf[16 + off: 16 + off + size].view(n, 4, 5, 11, 11)
                got, vattrs, eattrs = env.observe(dtype="codes", view_radius=radius, out=out, attrs=off == 0)
                assert got.data_ptr() == out.data_ptr()
                assert np.array_equal(got.cpu().numpy(), want), (radius, off)
                assert (buf[: 16 + off] == 0xAB).all() and (buf[16 + off + size:] == 0xAB).all(), (radius, off)
                if off == 0:
                    assert np.array_equal(vattrs.cpu().numpy(), vo.viewer_attrs(case["attrs"], case["env2"][:, 0])), radius
                    e = eattrs.cpu().numpy()
                    assert np.array_equal(e[:, :2], case["env2"])
                    assert np.array_equal(e[:, 2] & 1, st["done"]) and np.array_equal((e[:, 2] >> 1) & 1, st["draw"])
                    assert np.array_equal(e[:, 3], st["winner"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "float16", "float32"])
def test_plane_views_match_the_oracle(hip_lib, dtype):
    """radius 4 on the stress states, all three element types (n = 203: a last tile with an odd number of envs — the export stages
    two at a time)"""
    ob = _ob()
    case = _case("stress", 203, 23)
    _fog_is_tested(case, 4)
    planes, _, _ = ob.observe(case["states"], per_agent=True, dtype=getattr(np, dtype))
    want = vo.view_planes(planes, case["attrs"], 4)
    with _env(case["states"]) as env:
        got, vattrs, eattrs = env.observe(dtype=dtype, view_radius=4)
        assert got.shape == (203, 4, 16, 11, 11) and got.dtype.itemsize == np.dtype(dtype).itemsize
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(vattrs.cpu().numpy(), vo.viewer_attrs(case["attrs"], case["env2"][:, 0]))
        assert np.array_equal(eattrs.cpu().numpy()[:, :2], case["env2"])
        again, a, e = env.observe(dtype=dtype, view_radius=4, per_agent=True, attrs=False, out=got)
        assert a is None and e is None and again.data_ptr() == got.data_ptr() and np.array_equal(again.cpu().numpy(), want)
        with pytest.raises(ValueError):
            env.observe(dtype=dtype, view_radius=4, per_agent=False)
        with pytest.raises(ValueError):
            env.observe(dtype=dtype, view_radius=11)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks,n", [("stress", 23, 200), ("ffa", 57, 67)])
def test_radius_10_is_the_unfogged_output(hip_lib, kind, ticks, n):
    """against the existing calls, not the oracle"""
    case = _case(kind, n, ticks)
    with _env(case["states"]) as env:
        for dtype in ("uint8", "float16", "float32"):
            plain, _, _ = env.observe(per_agent=True, dtype=dtype, attrs=False)
            got, _, _ = env.observe(dtype=dtype, view_radius=10, attrs=False)
            assert got.shape == plain.shape and (got == plain).all(), dtype
        codes, _, _ = env.observe(dtype="codes", attrs=False)
        views, _, _ = env.observe(dtype="codes", view_radius=10, attrs=False)
        for v in range(4):
            assert (views[:, v] == codes).all(), v


@pytest.mark.gpu
@pytest.mark.parametrize("at_end,fresh", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("dtype", ["codes", "uint8"])
def test_step_and_views_in_one_launch(hip_lib, at_end, fresh, dtype):
    """pom_batch_step_device_observe_view equals pom_batch_step_device followed by pom_batch_observe_view, bit for bit, through
    ticks in which envs restart (max_steps 9)"""
    import torch
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END
    n, cap = 300 + 13, 9
    kw = dict(mode=MODE_ENV, auto_reset=RESET_AT_END if at_end else True, max_steps=cap, fresh_boards=fresh, board_seed=5)
    rng = np.random.default_rng(4)
    with BatchEnvironment(n, **kw) as env, BatchEnvironment(n, **kw) as twin:
        for e in (env, twin):
            if fresh:
                e.generate(5)
            else:
                e.make_game(pa.make_boards(n, seed=8, kind="stress"))
        restarts = 0
        for t in range(22):
            mv = torch.from_numpy(rng.integers(0, 6, size=(n, 4), dtype=np.int32)).to("cuda")
            got, vattrs, eattrs = env.step_device_observe(mv, dtype=dtype, view_radius=4)
            twin.step_device(mv)
            want, want_v, want_e = twin.observe(dtype=dtype, view_radius=4)
            assert env.get_state().tobytes() == twin.get_state().tobytes(), t
            assert (got == want).all() and (vattrs == want_v).all() and (eattrs == want_e).all(), t
            e = eattrs.cpu().numpy()
            if at_end:
                fin = env.last_results()["finished"]
                assert np.array_equal((e[:, 2] >> 3) & 1, fin), t
                restarts += int(fin.sum())
            else:
                restarts += int((e[:, 0] < t + 1).sum())   # a time step behind the ticks played: the env has started over
        assert restarts > 0
        assert np.array_equal(env.counters(), twin.counters())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["codes", "float16"])
def test_one_lane_shape_takes_the_two_launches(hip_lib, dtype):
    """a handle with one lane per env has no fused kernel: pom_batch_step_device_observe_view steps, then observes — the same
    outputs as the two calls, and as the quad shape's fused launch"""
    import torch
    from pomcpp_amd.batch import PomError
    case = _case("stress", 67, 23)
    mv = torch.from_numpy(np.random.default_rng(6).integers(0, 6, size=(67, 4), dtype=np.int32)).to("cuda")
    with _env(case["states"], lanes_per_env=1) as env, _env(case["states"], lanes_per_env=1) as twin, _env(case["states"]) as quad:
        for t in range(3):
            got, vattrs, eattrs = env.step_device_observe(mv, dtype=dtype, view_radius=4)
            twin.step_device(mv)
            want, want_v, want_e = twin.observe(dtype=dtype, view_radius=4)
            fused, fused_v, fused_e = quad.step_device_observe(mv, dtype=dtype, view_radius=4)
            assert env.get_state().tobytes() == twin.get_state().tobytes() == quad.get_state().tobytes(), t
            assert (got == want).all() and (vattrs == want_v).all() and (eattrs == want_e).all(), t
            assert (got == fused).all() and (vattrs == fused_v).all() and (eattrs == fused_e).all(), t
        out = torch.empty((67, 4, 5, 11, 11), dtype=torch.uint8, device="cuda")
        with pytest.raises(PomError):   # the range call is for the quad shape only, with or without views
            env.step_device_range(0, 67, mv, codes=out, view_radius=4)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["codes", "uint8"])
def test_range_writes_only_its_rows(hip_lib, dtype):
    """pom_batch_step_device_range_view over two ranges of a 90-env batch (six tiles, the last one partial): each call writes its
    range's rows of every array and nothing else; together they equal the step followed by pom_batch_observe_view"""
    import torch
    n, cut = 90, 48
    case = _case("stress", n, 23)
    per_view = 605 if dtype == "codes" else 1936
    mv = torch.from_numpy(np.random.default_rng(2).integers(0, 6, size=(n, 4), dtype=np.int32)).to("cuda")
    with _env(case["states"]) as env, _env(case["states"]) as twin:
        twin.step_device(mv)
        want, want_v, want_e = twin.observe(dtype=dtype, view_radius=4)
        out = torch.full((n, 4, per_view // 121, 11, 11), 0xAB, dtype=torch.uint8, device="cuda")
        vattrs = torch.full((n, 4, 12), -7, dtype=torch.int32, device="cuda")
        eattrs = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        env.sync()
        kw = dict(view_radius=4, viewer_attrs=vattrs, env_attrs=eattrs, **({"codes": out} if dtype == "codes" else {"planes": out}))
        env.step_device_range(0, cut, mv, **kw)
        env.sync()
        assert (out[:cut] == want[:cut]).all() and (vattrs[:cut] == want_v[:cut]).all() and (eattrs[:cut] == want_e[:cut]).all()
        assert (out[cut:] == 0xAB).all() and (vattrs[cut:] == -7).all() and (eattrs[cut:] == -7).all()
        env.step_device_range(cut, n - cut, mv, **kw)
        env.sync()
        assert (out == want).all() and (vattrs == want_v).all() and (eattrs == want_e).all()
        assert env.get_state().tobytes() == twin.get_state().tobytes()
        with pytest.raises(ValueError):                        # attribute arrays without views: nothing would write them
            env.step_device_range(0, n, mv, viewer_attrs=vattrs)
        with pytest.raises(ValueError):
            env.step_device_range(0, n, mv, view_radius=11, **{k: v for k, v in kw.items() if k != "view_radius"})
        with pytest.raises(ValueError):
            env.step_device_range(0, n, mv, view_radius=4, viewer_attrs=vattrs[:, :, :8].contiguous(), **{k: kw[k] for k in kw if k in ("codes", "planes")})
        env.step_device_range(0, n, mv, view_radius=None)     # no spec: the plain range step
        twin.step_device(mv)
        env.sync()
        assert env.get_state().tobytes() == twin.get_state().tobytes()


@pytest.mark.gpu
def test_bad_view_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header, with a message, and nothing written"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _ViewSpec
    n = 32
    case = _case("ffa", 67, 57)
    with _env(case["states"][:n].copy()) as env:
        lib, h = env._lib, env._h
        buf = torch.full((n * 4 * 1936 * 4 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        att = torch.full((n * 4 * 12 + 16,), -7, dtype=torch.int32, device="cuda")
        mv = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        size, p, a = C.sizeof(_ViewSpec), buf.data_ptr(), att.data_ptr()
        bad = {
            "struct_size": _ViewSpec(size - 8, 0, 4, 0, p, None, None),
            "dtype": _ViewSpec(size, 4, 4, 0, p, None, None),
            "radius -1": _ViewSpec(size, 0, -1, 0, p, None, None),
            "radius 11": _ViewSpec(size, 3, 11, 0, p, None, None),
            "reserved": _ViewSpec(size, 0, 4, 1, p, None, None),
            "null planes": _ViewSpec(size, 0, 4, 0, None, a, None),
            "uint8 planes + 1": _ViewSpec(size, 0, 4, 0, p + 1, None, None),
            "codes planes + 2": _ViewSpec(size, 3, 4, 0, p + 2, None, None),
            "half planes + 4": _ViewSpec(size, 1, 4, 0, p + 4, None, None),
            "float planes + 8": _ViewSpec(size, 2, 4, 0, p + 8, None, None),
            "viewer_attrs + 4": _ViewSpec(size, 0, 4, 0, p, a + 4, None),
            "env_attrs + 8": _ViewSpec(size, 0, 4, 0, p, None, a + 8),
        }
        calls = {
            "observe": lambda s: lib.pom_batch_observe_view(h, s),
            "fused": lambda s: lib.pom_batch_step_device_observe_view(h, mv.data_ptr(), s),
            "range": lambda s: lib.pom_batch_step_device_range_view(h, 0, n, mv.data_ptr(), None, s),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            for who, call in calls.items():
                with pytest.raises(PomError) as err:
                    _check(lib, call(C.byref(spec)))
                assert err.value.code != 0 and str(err.value), (what, who)
        for who in ("observe", "fused"):   # a null spec (the range call takes it for "no observation")
            with pytest.raises(PomError):
                _check(lib, calls[who](None))
        env.sync()
        assert (buf == 0xAB).all() and (att == -7).all()
        assert env.get_state().tobytes() == before   # and no refused call stepped
