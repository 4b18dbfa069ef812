"""The closed-loop range step (pom_batch_step_device_range) in every reset mode, with the ranges out of lockstep, against the host model
of a handle (tests/range_model.py) — bit for bit, everything the API can read: states, all six status arrays, episode numbers, all four
counters and, with POM_RESET_AT_END, the five arrays of last_results and the terminal records.

Shapes (tests/range_cases.py): 200 envs at env_offset 1000, twelve whole tiles and a short one of 8, cut into (0, 16) — a grid of one
workgroup —, (16, 144) — nine tiles, block0 != 0, more than one per XCD and a remainder modulo 8 — and (160, 40) — the short last tile,
up to the batch's end; one case of 40 envs.  What the schedules contain (restarts in every range, stale `finished` marks outside the
called range, whole tiles restarting, games that end by deaths, UB ticks) and that they tell five wrong kernels from a right one is
asserted without a GPU in tests/test_range_model_host.py."""
import numpy as np
import pytest

from pomcpp_amd.batch import BatchEnvironment, DIST_RANDOM, MODE_ENV, RESET_AT_END, RESET_AT_START
from tests import range_cases as RC

pytestmark = pytest.mark.gpu


def _handle(oracle, case):
    """the case's handle with its boards, settled"""
    env = BatchEnvironment(case["n"], **RC.options_of(case))
    start = RC.boards_of(oracle, case)
    if case["boards"] == "generated":
        env.generate(RC.BSEED)
        assert env.get_state().tobytes() == start.tobytes(), "generated boards"
    else:
        env.make_game(start)
    env.sync()
    return env


# ---- a. every mode against the model, after every call ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_every_mode_against_the_model_after_every_call(hip_lib, oracle, case):
    import torch
    model = RC.model_of(oracle, case)
    with _handle(oracle, case) as env:
        model.same_as(env, "before the first call")
        for j, (i, moves) in enumerate(RC.schedule(case)):
            first, count = case["ranges"][i]
            mv = torch.from_numpy(moves).to("cuda")   # one fresh device tensor per call (the copy from pageable memory has finished)
            env.step_device_range(first, count, mv)
            env.sync()
            model.tick(first, count, moves)
            model.same_as(env, f"{case['name']}: call {j}, range ({first}, {count})")


# ---- b. two streams, out of lockstep, no host wait in between ----------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.STREAM_CASES, ids=[c["name"] for c in RC.STREAM_CASES])
def test_two_streams_out_of_lockstep(hip_lib, oracle, case):
    """per round stream A carries three ticks of range 0 and two of range 2 while stream B carries one tick of range 1; nothing but
    the streams orders the calls, and one synchronisation ends the round"""
    import torch
    model = RC.model_of(oracle, case)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with _handle(oracle, case) as env:
        for r, (calls_a, calls_b) in enumerate(RC.stream_schedule(case)):
            tensors = [[torch.from_numpy(moves).to("cuda") for _, moves in calls] for calls in (calls_a, calls_b)]   # alive until the join
            for s in (a, b):
                s.wait_stream(torch.cuda.current_stream())   # the set-up: the moves' copies, and everything read back before
            for k in range(max(len(calls_a), len(calls_b))):   # issued alternately: neither stream's calls wait for the other's
                for s, calls, tens in ((a, calls_a, tensors[0]), (b, calls_b, tensors[1])):
                    if k < len(calls):
                        env.step_device_range(*case["ranges"][calls[k][0]], tens[k], s)
            torch.cuda.synchronize()
            for i, moves in calls_a + calls_b:
                model.tick(*case["ranges"][i], moves)
            model.same_as(env, f"{case['name']}: round {r}")
            del tensors


# ---- c. the fused observation of a range in every form the C entry takes -----------------------------------------------------------
FORMS = [(False, "uint8"), (True, "uint8"), (False, "float32"), (True, "float16"), (False, "codes")]


@pytest.mark.parametrize("per_agent,dtype", FORMS, ids=[f"{'per_agent' if p else 'shared'}-{d}" for p, d in FORMS])
def test_fused_observation_of_a_range_in_every_form(hip_lib, oracle, per_agent, dtype):
    """planes or codes, agent_attrs and env_attrs of the range's envs = the numpy restatement applied to the downloaded state, every
    tick, restarted envs included (max_steps 9, reset at the end of the tick); the rows outside the range keep their sentinel"""
    import torch
    from tests.test_observe import _oracle as observe_oracle
    ob, case = observe_oracle(), RC.OBS_CASE
    n = case["n"]
    model = RC.model_of(oracle, case)
    tdt = torch.uint8 if dtype == "codes" else getattr(torch, dtype)
    shape = (n, 5, 11, 11) if dtype == "codes" else (n, 4, 16, 11, 11) if per_agent else (n, 16, 11, 11)
    fill = 0xEE if tdt == torch.uint8 else -7.0
    restarted_seen = 0
    with _handle(oracle, case) as env:
        for j, (i, moves) in enumerate(RC.schedule(case, RC.OBS_ROUNDS)):
            first, count = case["ranges"][i]
            out = torch.full(shape, fill, dtype=tdt, device="cuda")
            a_attrs = torch.full((n, 4, 8), -7, dtype=torch.int32, device="cuda")
            e_attrs = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
            mv = torch.from_numpy(moves).to("cuda")
            torch.cuda.synchronize()   # the sentinels are in place before the handle's stream writes
            kw = dict(codes=out) if dtype == "codes" else dict(planes=out, per_agent=per_agent)
            env.step_device_range(first, count, mv, None, agent_attrs=a_attrs, env_attrs=e_attrs, **kw)
            env.sync()
            model.tick(first, count, moves)
            what = f"call {j}, range ({first}, {count})"
            model.same_as(env, what)
            states, st, fin = env.get_state(), env.status(), env.last_results()["finished"]
            if dtype == "codes":
                want, (_, want_a, want_e) = ob.observe_codes(states), ob.observe(states)
            else:
                want, want_a, want_e = ob.observe(states, per_agent=per_agent, dtype=getattr(np, dtype))
            inside = np.zeros(n, dtype=bool)
            inside[first:first + count] = True
            got, a, e = out.cpu().numpy(), a_attrs.cpu().numpy(), e_attrs.cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got[inside], want[inside]), what
            assert np.array_equal(a[inside], want_a[inside]), what
            assert np.array_equal(e[inside, :2], want_e[inside]), what
            assert np.array_equal(e[inside, 2] & 1, st["done"][inside]) and np.array_equal(e[inside, 3], st["winner"][inside]), what
            assert np.array_equal((e[inside, 2] >> 3) & 1, fin[inside]), what
            assert (got[~inside] == fill).all() and (a[~inside] == -7).all() and (e[~inside] == -7).all(), f"{what}: written outside the range"
            restarted_seen += int(fin[inside].sum())
    assert restarted_seen > n // 2, "precondition: restarted envs were observed"


# ---- d. next to chained calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settled", [False, True], ids=["no_sync_between", "read_back_between"])
@pytest.mark.parametrize("reset", [RESET_AT_START, RESET_AT_END], ids=["at_start", "at_end"])
def test_range_ticks_next_to_chained_calls(hip_lib, oracle, reset, settled):
    """a chained call, range ticks of all three ranges on the handle's stream straight behind it — the chained launches unsettled —, a
    chained call straight behind them; the second call's moves are those of tick 27: a range tick does not advance the handle's tick"""
    import torch
    case = RC.chain_case(reset)
    model = RC.model_of(oracle, case)
    ticks = RC.chain_range_ticks(case)
    with BatchEnvironment(case["n"], mode=MODE_ENV, auto_reset=reset, max_steps=case["cap"], env_offset=RC.ENV_OFFSET) as env:
        assert env.issue_info()[0] == "chain" and env.launch_shape() == (16, 4, 1), "a default handle of this size chains"
        env.make_game(RC.boards_of(oracle, case))
        tensors = [torch.from_numpy(moves).to("cuda") for _, moves in ticks]
        torch.cuda.synchronize()
        env.set_tick(RC.CHAIN_TICK0)
        env.step_random(RC.CHAIN_SEED, DIST_RANDOM, ticks=RC.CHAIN_TICKS)
        model.random_ticks(RC.CHAIN_SEED, DIST_RANDOM, RC.CHAIN_TICK0, RC.CHAIN_TICKS)
        if settled:
            model.same_as(env, "after the first chained call")
        for (i, moves), mv in zip(ticks, tensors):
            env.step_device_range(*case["ranges"][i], mv)
            model.tick(*case["ranges"][i], moves)
        if settled:
            model.same_as(env, "after the range ticks")
        env.step_random(RC.CHAIN_SEED, DIST_RANDOM, ticks=RC.CHAIN_TICKS)
        model.random_ticks(RC.CHAIN_SEED, DIST_RANDOM, RC.CHAIN_TICK0 + RC.CHAIN_TICKS, RC.CHAIN_TICKS)
        model.same_as(env, "after the second chained call")
        assert env.chain_stats()["tiles_recovered"] == 0
