"""The compact views (include/pom_batch.h PomCompactViewSpec) on the GPU: pom_batch_observe_view with the longer spec byte for byte
against the checker (tests/compact_view_oracle.py) applied to the numpy four-view oracle AND to the four-view kernel's output on the
same handle; the hand-made corner, edge and dead viewers in every tile column; step_mixed / step_events on twin handles, one writing
four views and one compact ones, through restarts in every FRESH / ATEND instantiation; a captured graph; the refusals.  Every
output lies between 0xAB guard bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import (BatchEnvironment, MODE_ENV, RESET_AT_END, RESET_AT_START, PomError, _check, _CompactViewSpec, _MixedStepSpec,
                              _StepEventsSpec, _ViewSpec, _spec)
from tests import compact_view_oracle as co
from tests import fog_columns as FC
from tests import view_oracle as vo
from tests.compact_view_cases import hand_states
from tests.test_observe_view import _case, _env, _ob

pytestmark = pytest.mark.gpu
GUARD = 64
MASKS = (1, 2, 4, 8, 5, 14, 15)
RADII = (0, 1, 4, 5, 10)


def _guarded(shape, dtype="uint8"):
    """(the tensor inside a larger 0xAB buffer, check()): the tensor 16-byte aligned, GUARD bytes of 0xAB before and after it"""
    import torch
    t = getattr(torch, dtype)
    item = torch.empty((), dtype=t).element_size()
    size = int(np.prod(shape)) * item
    buf = torch.full((GUARD + size + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
    out = buf[GUARD:GUARD + size].view(t).view(*shape)
    torch.cuda.synchronize()   # the handles' streams do not wait for torch's

    def intact():
        return bool((buf[:GUARD] == 0xAB).all() and (buf[GUARD + size:] == 0xAB).all())
    return out, intact


@functools.lru_cache(maxsize=None)
def _batch37():
    """37 envs — two full tiles and a tile of five whose last pass holds one env: the hand-made states, mid-game stress games, and
    the hand-made ones again at the end (env 36 is the one with the dead viewer).  With the unfogged numpy arrays; read only"""
    game, hand = _case("stress", 67, 23)["states"], hand_states()
    states = np.concatenate([hand, game[:31], hand])
    states["agents"]["pad"] = 0
    ob = _ob()
    _, attrs, env2 = ob.observe(states, per_agent=True)
    out = dict(states=states, attrs=attrs, env2=env2, codes=ob.observe_codes(states))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _four_views37(radius):
    case = _batch37()
    out = vo.view_codes(case["codes"], case["attrs"], radius)
    out.setflags(write=False)
    return out


# ---- 1. stand-alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centred", (False, True), ids=("uncentred", "centred"))
@pytest.mark.parametrize("radius", RADII)
def test_observe_view_against_the_oracle_and_the_four_view_kernel(hip_lib, radius, centred):
    case, n = _batch37(), 37
    want_four = _four_views37(radius)
    want_va = vo.viewer_attrs(case["attrs"], case["env2"][:, 0])
    with _env(case["states"]) as env:
        four, four_va, four_ea = env.observe(dtype="codes", view_radius=radius)
        four, four_va, four_ea = four.cpu().numpy(), four_va.cpu().numpy(), four_ea.cpu().numpy()
        assert np.array_equal(four, want_four) and np.array_equal(four_va, want_va)
        for mask in MASKS:
            k, s = bin(mask).count("1"), co.side(radius, centred)
            assert (n * k * 5 * s * s) % 2 == k % 2   # odd for odd k: the batch ends off a dword
            out, intact = _guarded((n, k, 5, s, s))
            # observe() allocates the attributes itself: hand it guarded ones through the spec instead
            va, va_intact = _guarded((n, k, 12), "int32")
            ea, ea_intact = _guarded((n, 4), "int32")
            spec = pa._abi._view_spec(3, radius, out, va, ea, compact=(mask, int(centred)))
            env.sync()
            _check(env._lib, env._lib.pom_batch_observe_view(env._h, C.byref(spec)))
            env.sync()
            got = out.cpu().numpy()
            assert np.array_equal(got, co.compact_codes(want_four, case["attrs"], radius, mask, centred)), (mask, "the numpy oracle")
            assert np.array_equal(got, co.compact_codes(four, four_va, radius, mask, centred)), (mask, "the four-view kernel")
            assert np.array_equal(va.cpu().numpy(), co.compact_viewer_attrs(four_va, mask)), mask
            assert np.array_equal(ea.cpu().numpy(), four_ea), mask
            assert intact() and va_intact() and ea_intact(), mask
        # the wrapper's own way: new tensors of the right shapes
        got, va, ea = env.observe(dtype="codes", view_radius=radius, viewers=[0, 2], centred=centred)
        assert np.array_equal(got.cpu().numpy(), co.compact_codes(want_four, case["attrs"], radius, 5, centred))
        assert np.array_equal(va.cpu().numpy(), co.compact_viewer_attrs(want_va, 5)) and np.array_equal(ea.cpu().numpy(), four_ea)
        assert env.get_state().tobytes() == case["states"].tobytes()


# ---- 2. every tile column -----------------------------------------------------------------------------------------------------------
def test_hand_made_viewers_in_every_tile_column(hip_lib):
    """the corner, edge and dead viewers in each of the 16 columns of a tile (so in each of the four passes, at each place in a pass),
    ordinary games around them; n = 21: a short last tile whose last pass holds one env"""
    n, hand, ob = 21, hand_states(), _ob()
    game = _case("stress", 67, 23)["states"]
    placements = [(FC.cases_of_slots(len(hand), r, n), 0) for r in range(16)]
    FC.check_columns(placements, len(hand))
    with BatchEnvironment(n, mode=MODE_ENV) as env:
        for r, (case_of_env, _) in enumerate(placements):
            states = game[:n].copy()
            states[FC.slots(len(hand), r)] = hand
            states["agents"]["pad"] = 0
            env.make_game(states)
            _, attrs, _env2 = ob.observe(states, per_agent=True)
            codes = ob.observe_codes(states)
            for mask, radius, centred in ((0b1011, 4, True), (0b0100, 1, False), (15, 0, True)):
                k, s = bin(mask).count("1"), co.side(radius, centred)
                out, intact = _guarded((n, k, 5, s, s))
                got, _, _ = env.observe(dtype="codes", view_radius=radius, viewers=mask, centred=centred, out=out, attrs=False)
                want = co.compact_codes(vo.view_codes(codes, attrs, radius), attrs, radius, mask, centred)
                assert np.array_equal(got.cpu().numpy(), want) and intact(), (r, mask, radius, centred)


# ---- 3. fused, on twin handles --------------------------------------------------------------------------------------------------------
def _read(env, at_end):
    out = dict(state=env.get_state(), episodes=env.episodes(), counters=env.counters(), memory=env.policy_memory())
    out.update({"status_" + k: v for k, v in env.status().items()})
    if at_end:
        out.update(terminal=env.get_terminal_state(), **{"last_" + k: v for k, v in env.last_results().items()})
    return out


def _twins(hip_lib, call, reset, fresh, viewers, centred, n, ranges):
    """`ranges`: [(first, count)] per tick.  Handle a writes four views, handle b compact ones; after every tick everything the API can
    read is the same, and b's output is the checker's of a's"""
    import torch
    radius, simple, at_end = 4, 0b1110, reset == RESET_AT_END
    mask = viewers if isinstance(viewers, int) else sum(1 << v for v in viewers)
    k, s = bin(mask).count("1"), co.side(radius, centred)
    options = dict(mode=MODE_ENV, auto_reset=reset, max_steps=6, fresh_boards=fresh, board_seed=13)
    rng = np.random.default_rng([3, reset, int(fresh), mask])
    with BatchEnvironment(n, **options) as a, BatchEnvironment(n, **options) as b:
        for h in (a, b):
            if fresh:
                h.generate(13)
            else:
                h.make_game(pa.make_boards(n, seed=8, kind="stress"))
            h.step_mixed(0, 0, None, 0xF, 1, 0)   # the agents' memory from the start
            h.sync()
        four, four_ok = _guarded((n, 4, 5, 11, 11))
        four_va, four_ea = torch.full((n, 4, 12), -7, dtype=torch.int32, device="cuda"), torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        out, out_ok = _guarded((n, k, 5, s, s))
        va, va_ok = _guarded((n, k, 12), "int32")
        ea, ea_ok = _guarded((n, 4), "int32")
        ev_a, ev_b = (torch.full((n, 4), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        stepped, restarts = np.zeros(n, dtype=bool), 0
        for t, (first, count) in enumerate(ranges):
            mv = torch.from_numpy(rng.integers(0, 6, size=(n, 4), dtype=np.int32)).to("cuda")
            torch.cuda.synchronize()
            kw_a = dict(codes=four, view_radius=radius, viewer_attrs=four_va, env_attrs=four_ea)
            kw_b = dict(codes=out, view_radius=radius, viewer_attrs=va, env_attrs=ea, viewers=viewers, centred=centred)
            if call == "mixed":
                a.step_mixed(first, count, mv, simple, 9, 100 + t, **kw_a)
                b.step_mixed(first, count, mv, simple, 9, 100 + t, **kw_b)
            else:
                a.step_events(first, count, mv, simple, 9, 100 + t, ev_a, **kw_a)
                b.step_events(first, count, mv, simple, 9, 100 + t, ev_b, **kw_b)
            ra, rb = _read(a, at_end), _read(b, at_end)
            bad = [key for key in ra if np.asarray(ra[key]).tobytes() != np.asarray(rb[key]).tobytes()]
            assert not bad, (t, bad)
            torch.cuda.synchronize()
            assert torch.equal(ev_a, ev_b), t
            stepped[first:first + count] = True
            f4, f4va = four.cpu().numpy(), four_va.cpu().numpy()
            got, got_va, got_ea = out.cpu().numpy(), va.cpu().numpy(), ea.cpu().numpy()
            assert np.array_equal(got[stepped], co.compact_codes(f4[stepped], f4va[stepped], radius, mask, centred)), t
            assert np.array_equal(got_va[stepped], co.compact_viewer_attrs(f4va[stepped], mask)), t
            assert np.array_equal(got_ea[stepped], four_ea.cpu().numpy()[stepped]), t
            assert (got[~stepped] == 0xAB).all() and (got_va[~stepped].view(np.uint8) == 0xAB).all() and (got_ea[~stepped].view(np.uint8) == 0xAB).all(), t
            assert four_ok() and out_ok() and va_ok() and ea_ok(), t
            restarts = int(ra["counters"][2])
        assert restarts > 0, "precondition: restarts (max_steps 6)"
        return stepped


@pytest.mark.parametrize("viewers,centred", (([0], True), (0b0101, False)), ids=("learner-centred", "two-uncentred"))
@pytest.mark.parametrize("fresh", (False, True), ids=("snapshot", "fresh"))
@pytest.mark.parametrize("reset", (RESET_AT_START, RESET_AT_END), ids=("at_start", "at_end"))
@pytest.mark.parametrize("call", ("mixed", "events"))
def test_fused_twins_four_views_and_compact_views(hip_lib, call, reset, fresh, viewers, centred):
    """n = 48: the range [16, 48) is stepped 12 ticks and [0, 16) once, in between; max_steps 6, so envs restart"""
    ranges = [(16, 32)] * 7 + [(0, 16)] + [(16, 32)] * 5
    stepped = _twins(hip_lib, call, reset, fresh, viewers, centred, 48, ranges)
    assert stepped.all()


@pytest.mark.parametrize("call", ("mixed", "events"))
def test_fused_short_last_tile(hip_lib, call):
    """n = 37, the range [32, 37): the short last tile inside a fused call, its last pass one env, the batch ending off a dword"""
    stepped = _twins(hip_lib, call, RESET_AT_END, False, [0], True, 37, [(32, 5)] * 8)
    assert stepped[32:].all() and not stepped[:32].any()


# ---- 4. a captured graph ------------------------------------------------------------------------------------------------------------
def test_three_captured_ticks_with_compact_views(hip_lib):
    import torch
    n, options = 48, dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=5, fresh_boards=True, board_seed=13)
    moves = [torch.from_numpy(np.random.default_rng(k).integers(0, 6, size=(n, 4), dtype=np.int32)).to("cuda") for k in range(3)]

    def outputs():
        return [dict(events=torch.full((n, 4), -7, dtype=torch.int32, device="cuda"), codes=torch.full((n, 1, 5, 9, 9), 0xAB, dtype=torch.uint8, device="cuda"),
                     viewer_attrs=torch.full((n, 1, 12), -7, dtype=torch.int32, device="cuda"),
                     env_attrs=torch.full((n, 4), -7, dtype=torch.int32, device="cuda")) for _ in range(3)]
    with BatchEnvironment(n, **options) as plain, BatchEnvironment(n, **options) as graphed:
        eager, replayed = outputs(), outputs()
        for h in (plain, graphed):
            h.generate(13)
            h.step_events(0, 0, None, 0xF, 1, 0, eager[0]["events"])   # count 0: allocates the agents' memory, writes nothing
            h.sync()
        torch.cuda.synchronize()
        main = torch.cuda.Stream()
        main.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=main):   # one stream, a single chain
            for t in range(3):
                graphed.step_events(0, n, moves[t], 0b1110, 6, 50 + t, stream=main, view_radius=4, viewers=[0], centred=True, **replayed[t])
        assert (replayed[0]["codes"] == 0xAB).all(), "the capture itself plays nothing"
        for rep in range(2):   # the second replay runs into max_steps 5: restarts inside the graph
            g.replay()
            torch.cuda.synchronize()
            for t in range(3):
                plain.step_events(0, n, moves[t], 0b1110, 6, 50 + t, view_radius=4, viewers=[0], centred=True, **eager[t])
            plain.sync()
            torch.cuda.synchronize()
            for t in range(3):
                for key in eager[t]:
                    assert torch.equal(eager[t][key], replayed[t][key]), (rep, t, key)
        assert not (eager[2]["codes"] == 0xAB).all()
        assert plain.get_state().tobytes() == graphed.get_state().tobytes() and plain.counters()[2] > 0


# ---- 5. the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call_and_write_nothing(hip_lib):
    import torch
    n = 32
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=40) as env:
        env.make_game(pa.make_boards(n, seed=8, kind="stress"))
        env.step_mixed(0, 0, None, 0xF, 1, 0)
        lib, h = env._lib, env._h
        buf = torch.full((n * 4 * 5 * 21 * 21 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        att = torch.full((n * 4 * 12 + 16,), -7, dtype=torch.int32, device="cuda")
        events = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        mv = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p, a = buf.data_ptr(), att.data_ptr()

        def compact(size=56, dtype=3, radius=4, reserved=0, planes=p, vattrs=a, eattrs=None, mask=1, flags=1, reserved2=0):
            return _CompactViewSpec(_ViewSpec(size, dtype, radius, reserved, planes, vattrs, eattrs), mask, flags, reserved2)
        bad = {
            "viewer_mask 0": compact(mask=0), "viewer_mask 16": compact(mask=16), "viewer_mask -1": compact(mask=-1),
            "flags 2": compact(flags=2), "flags 3": compact(flags=3), "reserved2_": compact(reserved2=1), "view.reserved_": compact(reserved=1),
            "dtype uint8": compact(dtype=0), "dtype float32": compact(dtype=2), "dtype 4": compact(dtype=4),
            "planes NULL": compact(planes=None), "planes + 2": compact(planes=p + 2), "planes + 1": compact(planes=p + 1),
            "viewer_attrs + 4": compact(vattrs=a + 4), "env_attrs + 8": compact(eattrs=a + 8),
            "radius 11": compact(radius=11), "radius -1": compact(radius=-1), "struct_size 48": compact(size=48),
        }

        def step(view):
            return _spec(_MixedStepSpec, 0b1110, 0, n, mv.data_ptr(), 1, 5, None, C.pointer(view), None, 0, 0, None, None, 0, 0)
        ev = _spec(_StepEventsSpec, 0, events.data_ptr(), None, None, 0)
        calls = {
            "pom_batch_observe_view": lambda s: lib.pom_batch_observe_view(h, C.byref(s.view)),
            "pom_batch_step_mixed": lambda s: lib.pom_batch_step_mixed(h, C.byref(step(s.view))),
            "pom_batch_step_events": lambda s: lib.pom_batch_step_events(h, C.byref(step(s.view)), C.byref(ev)),
        }
        core = {
            "pom_batch_step_device_observe_view": lambda s: lib.pom_batch_step_device_observe_view(h, mv.data_ptr(), C.byref(s.view)),
            "pom_batch_step_device_range_view": lambda s: lib.pom_batch_step_device_range_view(h, 0, n, mv.data_ptr(), None, C.byref(s.view)),
        }
        before = (env.get_state().tobytes(), env.counters().tolist(), env.policy_memory().tobytes())
        for what, spec in bad.items():
            for who, call in {**calls, **core}.items():
                assert lib.pom_batch_destroy(None) == 1   # another call's text
                rc = call(spec)
                text = lib.pom_last_error().decode()
                assert rc == 1 and text.startswith(who + ": ") and len(text) > len(who) + 2, (what, who, rc, text)
        good = compact()
        for who, call in core.items():   # the core unit's fused calls do not serve the compact form, and say who does
            assert lib.pom_batch_destroy(None) == 1
            rc = call(good)
            text = lib.pom_last_error().decode()
            assert rc == 1 and text.startswith(who + ": ") and "pom_batch_step_mixed" in text and "pom_batch_observe_view" in text, (who, text)
        env.sync()
        torch.cuda.synchronize()
        assert (buf == 0xAB).all() and (att == -7).all() and (events == -7).all()
        assert (env.get_state().tobytes(), env.counters().tolist(), env.policy_memory().tobytes()) == before
        for who, call in calls.items():   # the doctored specs are good ones
            _check(lib, call(good))
        env.sync()
        assert not (buf[:n * 405] == 0xAB).all() and (buf[n * 405:] == 0xAB).all() and env.counters()[0] == 2 * n
        with pytest.raises(PomError):
            _check(lib, calls["pom_batch_observe_view"](compact(mask=0)))
