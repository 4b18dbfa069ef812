"""pom_batch_step_events (include/pom_batch.h PomStepEventsSpec) on the GPU: the hand-made cases of tests/step_events_cases.py through
the kernel in every tile column and in a short last tile; twin handles, step_mixed on one and step_events on the other, equal in
everything the API can read and in the observation, over every instantiation of the kernel; the host model's record
(tests/step_events_oracle.py EventsModel) against the kernel's, every tick, bit for bit, over the games the CPU test has looked into
(tests/step_events_games.py); under POM_RESET_AT_END the outcome of every END tick against last_results(); a captured graph; and the
refusals.  Every handle has at most 48 envs."""
import ctypes as C

import numpy as np
import pytest

import pomcpp_amd
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, MODE_RAW, RESET_AT_END, RESET_AT_START, RESET_OFF, _MixedStepSpec, _StepEventsSpec, _spec
from tests import range_cases as RC
from tests import step_events_cases as SC
from tests import step_events_games as SG
from tests import step_events_oracle as EO
from tests.mixed_model import MixedModel

pytestmark = pytest.mark.gpu


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def _record(n):
    """the three arrays, every row holding the sentinel no call writes (int32 tensors: the words are read back as uint32)"""
    import torch
    sentinel = lambda v: int(np.array(v, np.uint32).view(np.int32))  # noqa: E731
    out = (torch.full((n, 4), sentinel(EO.SENTINEL_EVENTS), dtype=torch.int32, device="cuda"),
           torch.full((n,), sentinel(EO.SENTINEL_OUTCOME), dtype=torch.int32, device="cuda"),
           torch.full((n,), EO.SENTINEL_WOOD, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()   # the handles' streams do not wait for torch's: the fills have landed before any call can write
    return out


def _host(events, outcome, wood):
    import torch
    torch.cuda.synchronize()   # ... and the calls have finished before torch's stream reads
    return events.cpu().numpy().view(np.uint32), outcome.cpu().numpy().view(np.uint32), wood.cpu().numpy()


# ---- 1. the hand-made cases, in every column and in the short last tile -------------------------------------------------------------
N_CASES = 40   # two whole tiles and a short one of 8


def _placement(group, s, r):
    """which case of the group env e holds under shift s, pass r: over the 16 shifts every case of a pass sits in every column of its
    tile, over the passes in every tile"""
    return [(((e % 16) - s) % 16 + 16 * (e // 16 + r)) % len(group) for e in range(N_CASES)]


def test_the_placements_put_every_case_in_every_column_and_in_the_short_tile():
    for mode in ("env", "raw"):
        g = SC.group(mode)
        seen = {(i, e % 16, e // 16) for r in range(-(-len(g) // 16)) for s in range(16) for e, i in enumerate(_placement(g, s, r))}
        for i in range(len(g)):
            assert {c for j, c, _t in seen if j == i} == set(range(16)) and {t for j, _c, t in seen if j == i} == {0, 1, 2}, (mode, i)


@pytest.mark.parametrize("mode", ("env", "raw"))
def test_hand_made_cases_in_every_column(hip_lib, oracle, mode):
    group = SC.group(mode)
    built = [c[2](oracle)[0] for c in group]
    depth = max(len(c[3]) for c in group)
    with BatchEnvironment(N_CASES, mode=MODE_ENV if mode == "env" else MODE_RAW, auto_reset=RESET_OFF, max_steps=SC.CAP) as env:
        for r in range(-(-len(group) // 16)):
            for s in range(16):
                where = _placement(group, s, r)
                start = np.stack([built[i] for i in where])
                start["agents"]["pad"] = 0
                env.make_game(start)
                events, outcome, wood = _record(N_CASES)
                for t in range(depth):
                    ticks = [group[i][3][min(t, len(group[i][3]) - 1)] for i in where]
                    env.step_events(0, N_CASES, _dev([tk[0] for tk in ticks]), 0, 1, t, events, outcome, wood)
                    ev, oc, wd = _host(events, outcome, wood)
                    for e, i in enumerate(where):
                        if t < len(group[i][3]):
                            _moves, want_ev, want_oc, want_wd = group[i][3][t]
                            assert (ev[e].tolist(), int(oc[e]), int(wd[e])) == (list(want_ev), want_oc, want_wd), \
                                (group[i][0], f"env {e}, shift {s}, tick {t}", [hex(w) for w in ev[e]], hex(int(oc[e])), int(wd[e]))


def test_a_range_call_leaves_the_other_rows_alone(hip_lib, oracle):
    group = SC.group("env")
    where = _placement(group, 3, 0)
    start = np.stack([group[i][2](oracle)[0] for i in where])
    start["agents"]["pad"] = 0
    with BatchEnvironment(N_CASES, mode=MODE_ENV, auto_reset=RESET_OFF, max_steps=SC.CAP) as env:
        env.make_game(start)
        events, outcome, wood = _record(N_CASES)
        env.step_events(16, 16, _dev([group[i][3][0][0] for i in where]), 0, 1, 0, events, outcome, wood)
        ev, oc, wd = _host(events, outcome, wood)
        for e, i in enumerate(where):
            inside = 16 <= e < 32
            want = group[i][3][0][1:] if inside else ((EO.SENTINEL_EVENTS,) * 4, EO.SENTINEL_OUTCOME, EO.SENTINEL_WOOD)
            assert (ev[e].tolist(), int(oc[e]), int(wd[e])) == (list(want[0]), want[1], want[2]), (e, group[i][0])
        # ... and without the two optional arrays the events are the same
        env.make_game(start)
        alone, _, _ = _record(N_CASES)
        env.step_events(16, 16, _dev([group[i][3][0][0] for i in where]), 0, 1, 0, alone)
        assert np.array_equal(_host(alone, outcome, wood)[0], ev)


# ---- 2. twin handles: everything step_mixed leaves, step_events leaves ------------------------------------------------------------------
TWIN_TICKS, TWIN_CAP = 60, 20


def _observation(form, n):
    import torch
    if form == "none":
        return {}
    if form == "codes":
        return dict(codes=torch.zeros((n, 5, 11, 11), dtype=torch.uint8, device="cuda"),
                    agent_attrs=torch.zeros((n, 4, 8), dtype=torch.int32, device="cuda"), env_attrs=torch.zeros((n, 4), dtype=torch.int32, device="cuda"))
    return dict(codes=torch.zeros((n, 4, 5, 11, 11), dtype=torch.uint8, device="cuda"), view_radius=4,
                viewer_attrs=torch.zeros((n, 4, 12), dtype=torch.int32, device="cuda"), env_attrs=torch.zeros((n, 4), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("reset,fresh", RC.MODES, ids=[f"{('off', 'at_start', 'at_end')[r]}-{'fresh' if f else 'snapshot'}" for r, f in RC.MODES])
def test_twin_handles_step_mixed_and_step_events(hip_lib, oracle, reset, fresh):
    import torch
    n, boards = SG.N, SG.boards_of(oracle)
    options = dict(mode=MODE_ENV, auto_reset=reset, max_steps=TWIN_CAP, env_offset=RC.ENV_OFFSET, fresh_boards=fresh, board_seed=RC.BSEED)
    reader = MixedModel(oracle, boards, max_steps=TWIN_CAP, auto_reset=reset)   # (only read_handle() is used)
    rng = np.random.default_rng([5, reset, int(fresh)])
    for mask in (0, 0b1110, 15):
        for form in ("none", "codes", "views"):
            with BatchEnvironment(n, **options) as a, BatchEnvironment(n, **options) as b:
                for h in (a, b):
                    h.make_game(boards)
                    h.step_mixed(0, 0, None, 0xF, 1, 0)   # both have the agents' memory from the start
                obs_a, obs_b = _observation(form, n), _observation(form, n)
                events, outcome, wood = _record(n)
                for t in range(TWIN_TICKS):
                    mv = None if mask == 15 else _dev(rng.integers(0, 6, size=(n, 4)))
                    first, count = (16, 32) if t % 7 == 6 else (0, n)
                    a.step_mixed(first, count, mv, mask, 9, 100 + t, **obs_a)
                    b.step_events(first, count, mv, mask, 9, 100 + t, events, outcome if mask else None, wood if mask else None, **obs_b)
                    torch.cuda.synchronize()
                    for k in obs_a:
                        assert k == "view_radius" or torch.equal(obs_a[k], obs_b[k]), (mask, form, t, k)
                ra, rb = reader.read_handle(a), reader.read_handle(b)
                bad = [k for k in ra if np.asarray(ra[k]).tobytes() != np.asarray(rb[k]).tobytes()]
                assert not bad and ra["counters"][0] > 0, (mask, form, bad)
                assert reset == RESET_OFF or ra["counters"][2] > 0, "precondition: restarts"
                assert (events.cpu().numpy().view(np.uint32) != EO.SENTINEL_EVENTS).all()


# ---- 3. the model's record against the kernel's, every tick ------------------------------------------------------------------------------
@pytest.mark.parametrize("game", SG.GAMES, ids=SG.GAME_IDS)
def test_the_models_record_against_the_kernels_every_tick(hip_lib, oracle, game):
    played = SG.play(oracle, game)
    with BatchEnvironment(SG.N, **SG.options_of(game)) as env:
        env.make_game(SG.boards_of(oracle))
        events, outcome, wood = _record(SG.N)
        for t, ((first, count, moves, tick), want) in enumerate(zip(SG.calls_of(game), played["ticks"])):
            env.step_events(first, count, _dev(moves), game["mask"], SG.SEED, tick, events, outcome, wood)
            ev, oc, wd = _host(events, outcome, wood)
            for name, got in (("events", ev), ("outcome", oc), ("wood", wd)):
                if not np.array_equal(got, want[name]):
                    e = int(np.nonzero((got != want[name]).reshape(SG.N, -1).any(1))[0][0])
                    raise AssertionError(f"{game['name']}: tick {t}, range ({first}, {count}): {name} of env {e}: "
                                         f"{[hex(int(v)) for v in np.atleast_1d(got[e])]} != {[hex(int(v)) for v in np.atleast_1d(want[name][e])]}")
        played["model"].same_as(env, game["name"])


# ---- 4. POM_RESET_AT_END: the outcome of an END tick is what last_results() reports, and the observation shows the new game ----------
def test_at_end_the_outcome_is_last_results_and_the_observation_is_the_new_game(hip_lib, oracle):
    import torch
    n, game = SG.N, SG._game(RESET_AT_END, False, 25, 0b1110)
    rng, ends = np.random.default_rng(8), 0
    with BatchEnvironment(n, **SG.options_of(game)) as env:
        start = SG.boards_of(oracle)
        env.make_game(start)
        events, outcome, wood = _record(n)
        env_attrs = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        codes, agent_attrs = torch.zeros((n, 5, 11, 11), dtype=torch.uint8, device="cuda"), torch.zeros((n, 4, 8), dtype=torch.int32, device="cuda")
        for t in range(60):
            env.step_events(0, n, _dev(rng.integers(0, 6, size=(n, 4))), game["mask"], 4, t, events, outcome, wood, codes=codes,
                            agent_attrs=agent_attrs, env_attrs=env_attrs)
            ev, oc, _ = _host(events, outcome, wood)
            last, attrs, alive_now = env.last_results(), env_attrs.cpu().numpy(), agent_attrs.cpu().numpy()[:, :, 2]
            end = (ev[:, 0] & EO.END) != 0
            assert np.array_equal(end, last["finished"] != 0) and ((ev & EO.END) != 0).all(1).tolist() == end.tolist()
            d = pomcpp_amd.decode_rollout(oc[end])
            assert d["done"].all() and np.array_equal(d["winner"], last["winner"][end]) and np.array_equal(d["draw"], last["draw"][end] != 0)
            assert np.array_equal(d["length"], last["length"][end]) and np.array_equal(d["alive"].sum(1), last["alive"][end])
            assert np.array_equal(d["timeout"], last["length"][end] >= game["cap"])
            won = (ev[end] & EO.WON) != 0
            assert np.array_equal(won, np.arange(4)[None, :] == last["winner"][end][:, None])
            # the observation of the same launch: the start state again, nobody has won, only the restarted bit
            assert np.array_equal(attrs[end], np.stack([start["timeStep"], start["aliveAgents"], np.full(n, 8), np.full(n, -1)], 1)[end])
            assert np.array_equal(alive_now[end], 1 - start["agents"]["dead"][end])
            assert (attrs[~end, 2] == 0).all()
            ends += int(end.sum())
    assert ends > n   # time-outs at 25 and natural ends


# ---- 5. a captured graph ---------------------------------------------------------------------------------------------------------------
def test_three_captured_ticks_replay_to_the_words_of_three_plain_calls(hip_lib, oracle):
    import torch
    n, game = SG.N, SG._game(RESET_AT_END, True, 5, 0b1110)
    moves = [_dev(np.random.default_rng(k).integers(0, 6, size=(n, 4))) for k in range(3)]
    with BatchEnvironment(n, **SG.options_of(game)) as plain, BatchEnvironment(n, **SG.options_of(game)) as graphed:
        records = [[_record(n) for _ in range(3)] for _ in range(2)]
        for h in (plain, graphed):
            h.make_game(SG.boards_of(oracle))
            h.step_events(0, 0, None, 0xF, 1, 0, records[0][0][0])   # count 0: allocates the agents' memory, writes nothing
            h.sync()
        main = torch.cuda.Stream()
        main.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=main):   # one stream, no parallel branches
            for t in range(3):
                graphed.step_events(0, n, moves[t], game["mask"], 6, 50 + t, *records[1][t], main)
        assert (records[1][0][0].cpu().numpy().view(np.uint32) == EO.SENTINEL_EVENTS).all(), "the capture itself plays nothing"
        for rep in range(2):   # the second replay runs into max_steps 5: END ticks and restarts inside the graph
            g.replay()
            torch.cuda.synchronize()
            for t in range(3):
                plain.step_events(0, n, moves[t], game["mask"], 6, 50 + t, *records[0][t])
            torch.cuda.synchronize()
            for t in range(3):
                for a, b in zip(records[0][t], records[1][t]):
                    assert torch.equal(a, b), (rep, t)
        assert any(((r[0].cpu().numpy().view(np.uint32) & EO.END) != 0).any() for r in records[0])
        assert plain.get_state().tobytes() == graphed.get_state().tobytes()


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call_and_launch_nothing(hip_lib, oracle):
    n = SG.N
    mv = _dev(np.zeros((n, 4)))
    events, outcome, wood = _record(n)

    def step(**kw):
        s = _spec(_MixedStepSpec, 0b1110, 0, 16, mv.data_ptr(), 1, 5, None, None, None, 0, 0, None, None, 0, 0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def ev(**kw):
        s = _spec(_StepEventsSpec, 0, events.data_ptr(), outcome.data_ptr(), wood.data_ptr(), 0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    rows = [("struct_size", step(), ev(struct_size=48)), ("flags", step(), ev(flags=1)), ("reserved_", step(), ev(reserved_=1)),
            ("events NULL", step(), ev(events_dev=None)), ("events misaligned", step(), ev(events_dev=events.data_ptr() + 2)),
            ("outcome misaligned", step(), ev(outcome_dev=outcome.data_ptr() + 1)), ("a null events spec", step(), None),
            ("the step's mask", step(simple_mask=16), ev()), ("the step's range", step(first=8), ev()), ("the step's moves", step(moves_dev=None), ev()),
            ("the step's size", step(struct_size=96), ev())]
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=40) as env:
        env.make_game(SG.boards_of(oracle))
        before = (env.get_state().tobytes(), env.counters().tolist())
        texts = set()
        for what, s, e in rows:
            assert hip_lib.pom_batch_destroy(None) == 1   # another call's text
            rc = hip_lib.pom_batch_step_events(env._h, C.byref(s), None if e is None else C.byref(e))
            text = hip_lib.pom_last_error().decode()
            assert rc == 1 and text.startswith("pom_batch_step_events: "), (what, rc, text)
            texts.add(text)
        assert hip_lib.pom_batch_step_events(None, C.byref(step()), C.byref(ev())) == 1 and hip_lib.pom_last_error().decode().startswith("pom_batch_step_events: ")
        assert len(texts) == len(rows), texts
        env.sync()
        assert (env.get_state().tobytes(), env.counters().tolist()) == before
        assert (events.cpu().numpy().view(np.uint32) == EO.SENTINEL_EVENTS).all()
        assert hip_lib.pom_batch_step_events(env._h, C.byref(step()), C.byref(ev(outcome_dev=None, wood_dev=None))) == 0   # the doctored specs are good ones
        assert env.counters()[0] == 16
