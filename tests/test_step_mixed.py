"""pom_batch_step_mixed (include/pom_batch.h PomMixedStepSpec) on the GPU: the closed-loop range step with SimpleAgent for the agents of
a mask, against the host model of a handle (tests/mixed_model.py) — bit for bit, everything the API can read plus policy_memory() — in
every reset mode, for every mask, with the ranges out of lockstep and each range counting its own tick; on two streams; against the
existing calls where the header states an equivalence; with the fused observation in four forms; through the golden fixture that the
compiled reference played; and the things that must not change, the refusals and the graph capture.

Shapes (tests/mixed_cases.py, those of tests/range_cases.py): 200 envs at env_offset 1000 cut into (0, 16) — one workgroup —, (16, 144) —
nine tiles, block0 != 0 — and (160, 40) — the short last tile; cases of 40 envs.  What the schedules contain and that they tell six wrong
kernels from a right one is asserted without a GPU in tests/test_mixed_model_host.py."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.batch import (BatchEnvironment, DIST_RANDOM, MODE_ENV, RESET_AT_END, RESET_AT_START, RESET_OFF, PomError, _MixedStepSpec,
                              _spec, _view_spec)
from pomcpp_amd.state import STATE_DTYPE
from tests import mixed_cases as MC
from tests import range_cases as RC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixed_step.npz")


def _handle(oracle, case, pre=True):
    """the case's handle with its boards and, with `pre`, its PRE ticks of step_simple behind it; settled"""
    env = BatchEnvironment(case["n"], **RC.options_of(case))
    start = MC.boards_of(oracle, case)
    if case["boards"] == "generated":
        env.generate(RC.BSEED)
        assert env.get_state().tobytes() == start.tobytes(), "generated boards"
    else:
        env.make_game(start)
    if pre:
        env.set_tick(MC.PRE_TICK0)
        env.step_simple(MC.SEED, MC.PRE)
    env.sync()
    return env


def _dev(moves):
    import torch
    return torch.from_numpy(np.ascontiguousarray(moves, dtype=np.int32)).to("cuda")   # (the copy from pageable memory has finished)


# ---- 1. every case and mask against the model, after every call --------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.CASES, ids=MC.CASE_IDS)
def test_every_case_against_the_model_after_every_call(hip_lib, oracle, case):
    model = MC.model_of(oracle, case)
    with _handle(oracle, case) as env:
        model.same_as(env, "after the step_simple ticks")
        for j, (i, moves, tick) in enumerate(MC.schedule(case)):
            first, count = case["ranges"][i]
            mv = _dev(moves)
            env.step_mixed(first, count, mv, case["mask"], MC.SEED, tick)
            env.sync()
            model.tick_mixed(first, count, moves, case["mask"], MC.SEED, tick)
            model.same_as(env, f"{case['name']}: call {j}, range ({first}, {count}), tick {tick}")


# ---- 2. two streams, out of lockstep, nothing but the streams ordering the calls -----------------------------------------------------
@pytest.mark.parametrize("case", MC.STREAM_CASES, ids=[c["name"] for c in MC.STREAM_CASES])
def test_two_streams_out_of_lockstep(hip_lib, oracle, case):
    """per round stream A carries three ticks of range 0 and two of range 2 while stream B carries one tick of range 1, every range on
    its own tick counter; one synchronisation ends the round"""
    import torch
    model = MC.model_of(oracle, case)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with _handle(oracle, case) as env:
        for r, (calls_a, calls_b) in enumerate(MC.stream_schedule(case)):
            tensors = [[_dev(moves) for _, moves, _ in calls] for calls in (calls_a, calls_b)]   # alive until the join
            for s in (a, b):
                s.wait_stream(torch.cuda.current_stream())
            for k in range(max(len(calls_a), len(calls_b))):   # issued alternately: neither stream's calls wait for the other's
                for s, calls, tens in ((a, calls_a, tensors[0]), (b, calls_b, tensors[1])):
                    if k < len(calls):
                        env.step_mixed(*case["ranges"][calls[k][0]], tens[k], case["mask"], MC.SEED, calls[k][2], s)
            torch.cuda.synchronize()
            for i, moves, tick in calls_a + calls_b:
                model.tick_mixed(*case["ranges"][i], moves, case["mask"], MC.SEED, tick)
            model.same_as(env, f"{case['name']}: round {r}")
            del tensors


# ---- 3. the equivalences of the header, on twin handles ------------------------------------------------------------------------------
def _mode_case(reset, fresh):
    return MC._case(reset, fresh, 0, 6, "generated") if fresh else MC._case(reset, fresh, 0, 40, "burned")


def _read(model, env):
    return model.read_handle(env)


def _same(model, a, b, what, but=()):
    ra, rb = _read(model, a), _read(model, b)
    bad = [k for k in ra if k not in but and np.asarray(ra[k]).tobytes() != np.asarray(rb[k]).tobytes()]
    assert not bad, f"{what}: {bad} differ"
    return ra, rb


@pytest.mark.parametrize("reset,fresh", RC.MODES, ids=[f"{('off', 'at_start', 'at_end')[r]}-{'fresh' if f else 'snapshot'}" for r, f in RC.MODES])
def test_equivalences_on_twin_handles(hip_lib, oracle, reset, fresh):
    import torch
    case = _mode_case(reset, fresh)
    n, rng = case["n"], np.random.default_rng(31)
    model = MC.model_of(oracle, case, pre=False)   # (only its readers are used)
    # mask 0 is the range call, bit for bit — range by range, the ranges at different ticks
    with _handle(oracle, case) as a, _handle(oracle, case) as b:
        for j in range(12):
            first, count = case["ranges"][(0, 1, 2, 1, 2, 2)[j % 6]]
            mv = _dev(rng.integers(0, 6, size=(n, 4)))
            before, done_before = a.policy_memory(), a.status()["done"].astype(bool)
            a.step_mixed(first, count, mv, 0, MC.SEED, 77 + j)
            b.step_device_range(first, count, mv)
            ra, _ = _same(model, a, b, f"mask 0, call {j}", but=("memory",))
            # the range call knows nothing of the agents' memory; this one asks nobody and wipes the memory of the envs it restarts
            restarted = done_before if reset == RESET_AT_START else ra["last_finished"].astype(bool) if reset == RESET_AT_END else np.zeros(n, bool)
            restarted[:first], restarted[first + count:] = False, False
            assert np.array_equal(ra["memory"], np.where(restarted[:, None, None], 0, before)), f"mask 0, call {j}: memory"
        assert reset == RESET_OFF or a.counters()[2] > 0, "precondition: restarts"
    # any mask, whole batch: set_tick, policy_simple, the other agents' entries overwritten, step_policy.  With POM_RESET_AT_END the
    # sequence's tick has no policy in it and leaves the memory of an env it restarts as it was, where this call wipes it (step 5 of the
    # header, as step_simple): there the twins are compared up to and including the first tick that restarts an env, from two starts
    for mask, warm in ((0b1110, 0), (0b0101, 0)) + (((0b1110, 3),) if reset == RESET_AT_END else ()):
        with _handle(oracle, case) as a, _handle(oracle, case) as b:
            keep = torch.tensor([bool(mask >> k & 1) for k in range(4)], device="cuda")
            in_mask = np.array([bool(mask >> k & 1) for k in range(4)])
            for j in range(warm):   # the same mixed ticks on both
                mv = _dev(rng.integers(0, 6, size=(n, 4)))
                for h in (a, b):
                    h.step_mixed(0, n, mv, mask, MC.SEED, 4000 + j)
                torch.cuda.synchronize()
            restarts = 0
            for j in range(12):
                tick = 5000 + 3 * j
                mv = _dev(rng.integers(0, 6, size=(n, 4)))
                before, done_before = a.policy_memory(), a.status()["done"].astype(bool)
                a.step_mixed(0, n, mv, mask, MC.SEED, tick)
                b.set_tick(tick)
                b.policy_simple(MC.SEED)
                b.sync()
                buf = b.moves_tensor()
                buf.copy_(torch.where(keep, buf, mv))
                torch.cuda.synchronize()
                del buf
                b.step_policy()
                ra, rb = _same(model, a, b, f"mask {mask:#x}, tick {j}", but=("memory",))
                at_start = done_before if reset == RESET_AT_START else np.zeros(n, bool)
                at_end = ra["last_finished"].astype(bool) if reset == RESET_AT_END else np.zeros(n, bool)
                restarts += int(at_start.sum() + at_end.sum())
                want_mask = np.where(at_end[:, None, None], 0, rb["memory"])
                assert np.array_equal(ra["memory"][:, in_mask], want_mask[:, in_mask]), f"mask {mask:#x}, tick {j}: the mask's agents' memory"
                want = np.where((at_start | at_end)[:, None, None], 0, before)
                assert np.array_equal(ra["memory"][:, ~in_mask], want[:, ~in_mask]), f"mask {mask:#x}, tick {j}: the other agents' memory"
                if at_end.any():
                    break
            assert reset == RESET_OFF or restarts > 0, "precondition: restarts"
    # all four agents, whole batch: set_tick and one step_simple tick, bit for bit, memory included (moves may be None)
    with _handle(oracle, case) as a, _handle(oracle, case) as b:
        for j in range(12):
            a.step_mixed(0, n, None, 0xF, MC.SEED, 900 + 2 * j)
            b.set_tick(900 + 2 * j)
            b.step_simple(MC.SEED, 1)
            _same(model, a, b, f"mask 0xF, tick {j}")


# ---- 4. the fused observation is the call without it followed by observe ---------------------------------------------------------------
FORMS = [("codes", False, None), ("float16", True, None), ("codes", True, 4), ("uint8", True, 0)]


@pytest.mark.parametrize("dtype,per_agent,radius", FORMS, ids=["shared-codes", "per_agent-float16", "fogged-codes-r4", "fogged-uint8-r0"])
def test_fused_observation_is_the_call_followed_by_observe(hip_lib, oracle, dtype, per_agent, radius):
    import torch
    case = MC._case(RESET_AT_END, False, 0b1110, 6, "burned")   # restarted envs are observed
    n, view = case["n"], radius is not None
    tdt = torch.uint8 if dtype == "codes" else getattr(torch, dtype)
    depth = 5 if dtype == "codes" else 16
    shape = (n, 4, depth, 11, 11) if per_agent else (n, depth, 11, 11)
    fill = 0xEE if tdt == torch.uint8 else -7.0
    model = MC.model_of(oracle, case, pre=False)
    restarted_seen = 0
    with _handle(oracle, case) as a, _handle(oracle, case) as b:
        for j, (i, moves, tick) in enumerate(MC.schedule(case, 6)):
            first, count = case["ranges"][i]
            out = torch.full(shape, fill, dtype=tdt, device="cuda")
            attrs = torch.full((n, 4, 12 if view else 8), -7, dtype=torch.int32, device="cuda")
            e_attrs = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
            mv = _dev(moves)
            torch.cuda.synchronize()   # the sentinels are in place before the handle's stream writes
            kw = dict(codes=out) if dtype == "codes" else dict(planes=out)
            kw.update(dict(view_radius=radius, viewer_attrs=attrs) if view else dict(agent_attrs=attrs, per_agent=per_agent))
            a.step_mixed(first, count, mv, case["mask"], MC.SEED, tick, None, env_attrs=e_attrs, **kw)
            b.step_mixed(first, count, mv, case["mask"], MC.SEED, tick)
            want, want_a, want_e = b.observe(per_agent=None if view else per_agent, dtype=dtype, view_radius=radius)
            torch.cuda.synchronize()
            what = f"call {j}, range ({first}, {count})"
            ra, _ = _same(model, a, b, what)
            inside = torch.zeros(n, dtype=torch.bool, device="cuda")
            inside[first:first + count] = True
            assert out.dtype == want.dtype and torch.equal(out[inside], want[inside]), what
            assert torch.equal(attrs[inside], want_a[inside]) and torch.equal(e_attrs[inside], want_e[inside]), what
            assert bool((out[~inside] == fill).all()) and bool((attrs[~inside] == -7).all()) and bool((e_attrs[~inside] == -7).all()), \
                f"{what}: written outside the range"
            restarted_seen += int(ra["last_finished"][first:first + count].sum())
    assert restarted_seen > 0, "precondition: restarted envs were observed"


# ---- 5. the golden fixture through the GPU ------------------------------------------------------------------------------------------------
def test_golden_fixture(hip_lib):
    """every tick of it was played by the compiled reference's Step and every act by its SimpleAgent (tests/golden/gen_mixed_step.py)"""
    g = np.load(GOLDEN)
    start = np.ascontiguousarray(g["start"]).view(STATE_DTYPE).reshape(-1)
    n, mask, seed, tick0 = start.size, int(g["mask"]), int(g["seed"]), int(g["tick0"])
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=int(g["max_steps"]), env_offset=int(g["env_offset"])) as env:
        env.make_game(start)
        env.sync()
        for t in range(g["moves"].shape[0]):
            env.step_mixed(0, n, _dev(g["moves"][t]), mask, seed, tick0 + t)
            assert env.get_state().tobytes() == g["states"][t].tobytes(), f"tick {t}: states"
            assert np.array_equal(env.policy_memory(), g["mems"][t]), f"tick {t}: memory"
        assert env.counters()[2] == int(g["restarts"])


# ---- 6. nothing else changes ----------------------------------------------------------------------------------------------------------------
def test_nothing_else_changes(hip_lib, oracle):
    """the handle's tick (a following step_random draws what the model draws at the tick the step_simple ticks left), the handle's move
    buffer byte for byte, the envs outside the range"""
    import torch
    case = MC._case(RESET_AT_START, False, 0b0101, 40, "burned")
    n = case["n"]
    model = MC.model_of(oracle, case)
    with _handle(oracle, case) as env:
        buf = env.moves_tensor()
        buf.copy_(_dev(np.random.default_rng(8).integers(1, 6, size=(n, 4))))   # something in the move buffer
        torch.cuda.synchronize()
        buf_before = buf.clone()
        assert int(buf_before.abs().sum()) > 0
        for j, (i, moves, tick) in enumerate(MC.schedule(case, 3)):
            first, count = case["ranges"][i]
            state_before = env.get_state()
            env.step_mixed(first, count, _dev(moves), case["mask"], MC.SEED, tick)
            model.tick_mixed(first, count, moves, case["mask"], MC.SEED, tick)
            outside = np.ones(n, bool)
            outside[first:first + count] = False
            assert env.get_state()[outside].tobytes() == state_before[outside].tobytes(), f"call {j}: envs outside the range"
        torch.cuda.synchronize()
        assert torch.equal(buf, buf_before), "the handle's move buffer"
        del buf, buf_before
        # restarts of a policy-less tick leave the agents' memory alone: everything but the memory is compared
        env.step_random(MC.SEED, DIST_RANDOM, 2)
        model.random_ticks(MC.SEED, DIST_RANDOM, model.handle_tick, 2)
        bad = [k for k in model.differences(model.read_handle(env)) if k != "memory"]
        assert not bad, f"after step_random at the handle's own tick: {bad} differ"
        # ... and a handle whose tick a mixed call had moved would have drawn other moves
        right, wrong = MC.model_of(oracle, case), MC.model_of(oracle, case)
        right.random_ticks(MC.SEED, DIST_RANDOM, right.handle_tick, 2)
        wrong.random_ticks(MC.SEED, DIST_RANDOM, MC.RANGE_TICK0[0] + 1, 2)
        assert "state" in right.differences(wrong)


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib, oracle):
    import torch
    case = MC._case(RESET_AT_START, False, 0b1110, 40, "burned", RC.SMALL_N, RC.SMALL_RANGES)
    n = case["n"]
    mv = _dev(np.zeros((n, 4)))
    planes = torch.zeros((n, 4, 16, 11, 11), dtype=torch.uint8, device="cuda")
    codes = torch.zeros((n, 5, 11, 11), dtype=torch.uint8, device="cuda")
    e_attrs = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    size = C.sizeof(_MixedStepSpec)
    good_view = _view_spec(0, 4, planes)

    def spec(**kw):
        s = _spec(_MixedStepSpec, 0b1110, 0, 16, mv.data_ptr(), MC.SEED, 5, None, None, None, 0, 0, None, None, 0, 0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    rows = [
        ("struct_size 0", spec(struct_size=0)), ("struct_size + 8", spec(struct_size=size + 8)),
        ("simple_mask -1", spec(simple_mask=-1)), ("simple_mask 16", spec(simple_mask=16)),
        ("tick -1", spec(tick=-1)), ("tick 2^32", spec(tick=1 << 32)), ("flags", spec(flags=1)), ("reserved_", spec(reserved_=1)),
        ("moves NULL, mask 14", spec(moves_dev=None)), ("moves NULL, mask 0", spec(moves_dev=None, simple_mask=0)),
        ("moves misaligned", spec(moves_dev=mv.data_ptr() + 2)),
        ("first not a tile", spec(first=8, count=16)), ("count not whole tiles", spec(count=8)), ("past the batch", spec(first=32, count=16)),
        ("first < 0", spec(first=-16)), ("count < 0", spec(count=-16)),
        ("unknown dtype", spec(planes_dev=planes.data_ptr(), dtype=7)),
        ("codes per agent", spec(planes_dev=codes.data_ptr(), dtype=3, per_agent=1)),
        ("planes misaligned", spec(planes_dev=planes.data_ptr() + 1, dtype=0)),
        ("view radius 11", spec(view=C.pointer(_view_spec(0, 11, planes)))),
        ("view without planes", spec(view=C.pointer(_view_spec(0, 4, None)))),
        ("view and planes", spec(view=C.pointer(good_view), planes_dev=planes.data_ptr())),
        ("view and env_attrs", spec(view=C.pointer(good_view), env_attrs_dev=e_attrs.data_ptr())),
    ]
    lib = hip_lib

    def refused(h, s, what):
        assert lib.pom_batch_destroy(None) == 1   # another call's text
        rc = lib.pom_batch_step_mixed(h, None if s is None else C.byref(s))
        text = lib.pom_last_error().decode()
        assert rc == 1 and text.startswith("pom_batch_step_mixed: "), (what, rc, text)
        return text

    with _handle(oracle, case) as env:
        before = (env.get_state().tobytes(), env.counters().tolist(), env.policy_memory().tobytes(), env.episodes().tobytes())
        texts = {refused(env._h, s, what) for what, s in rows}
        texts.add(refused(env._h, None, "a null spec"))
        texts.add(refused(None, spec(), "a null handle"))
        assert len(texts) >= 12, texts
        env.sync()
        assert (env.get_state().tobytes(), env.counters().tolist(), env.policy_memory().tobytes(), env.episodes().tobytes()) == before
        env.step_mixed(0, 16, mv, 0b1110, MC.SEED, 5)   # the spec the rows doctor is a good one
        assert env.counters()[0] == before[1][0] + 16
    with BatchEnvironment(64, lanes_per_env=1, envs_per_wave=64) as one_lane:
        one_lane.make_game(RC.boards_of(oracle, dict(boards="new", n=64)))
        refused(one_lane._h, spec(), "a launch shape other than the quad shape")
        with pytest.raises(PomError):
            one_lane.step_mixed(0, 64, _dev(np.zeros((64, 4))), 1, 0, 0)


# ---- 8. count == 0 prepares; a captured graph of two mixed calls ----------------------------------------------------------------------------
def test_count_0_prepares_and_a_graph_of_two_calls_replays(hip_lib, oracle):
    import torch
    case = MC._case(RESET_AT_END, True, 0b1110, 6, "generated", RC.SMALL_N, RC.SMALL_RANGES)
    n = case["n"]
    model = MC.model_of(oracle, case, pre=False)
    rng = np.random.default_rng(3)
    moves = [rng.integers(0, 6, size=(n, 4)).astype(np.int32) for _ in range(2)]
    with _handle(oracle, case, pre=False) as env:   # no policy call yet: the handle has no agents' memory
        model.same_as(env, "before")
        env.step_mixed(0, 0, None, 0xF, MC.SEED, 0)   # allocates and clears the memory, and nothing else
        env.step_mixed(16, 0, _dev(moves[0]), 0b0010, MC.SEED, 0)
        model.same_as(env, "after the calls with count == 0")
        tensors = [_dev(m) for m in moves]
        main = torch.cuda.Stream()
        main.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=main):   # one stream, no parallel branches
            for t, mv in enumerate(tensors):
                env.step_mixed(0, n, mv, case["mask"], MC.SEED, 40 + t, main)
        model.same_as(env, "the capture itself plays nothing")
        for rep in range(3):   # five ticks reach max_steps 6: the replays restart envs on generated boards
            g.replay()
            torch.cuda.synchronize()
            for t, m in enumerate(moves):
                model.tick_mixed(0, n, m, case["mask"], MC.SEED, 40 + t)
            model.same_as(env, f"replay {rep}")
        assert model.counters[2] > 0, "precondition: a replay restarts envs"
