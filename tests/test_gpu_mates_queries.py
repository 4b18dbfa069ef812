"""The mixed step and the search kernels beside chosen wavefront-mates.  tests/test_tile_mates.py chooses an env's company — a mate that
pushes 19 explosion frames over the claim maps, one that fills all 31 dwords of its map, columns that restart beside a chain going off —
but spreads that net under pom_step_kernel only.  Every kernel below embeds the same tick in an LDS array of its own, with extras of
its own over or behind the tick's scratch rows, and has so far met whatever company played games and the record-edge corpus gave it:
  pom_step_mixed_kernel      its own three restart paths; the policy's overlay rows AND the export's staging rows over rows 80..
  pom_rollout_policy_kernel  RP_ROWS, then the parked memory and tick-1 moves behind the tile; JOBS gathers the tile column by column
  pom_rollout_kernel, pom_move_safety_kernel   loops that run until the slowest mate is done
  pom_forecast_kernel        FC_STAGE_ROW: the first-flame-tick bytes start on the row behind the last claim byte
  pom_expand_kernel          job columns laid over a loaded tile, fused export rows
  pom_step_kernel<OBS, VIEW> the fogged export over the scratch rows
Here all of them answer for the batch of tests/mates_queries.py (test_tile_mates._whole: overlay, pairs, restart, crowd; 3,381 envs),
at the tick before each actor's decisive one, byte for byte against the checkers that exist (Oracle.step's solo traces,
tests/mixed_model.py, tests/*_oracle.py, oracle/pom_observe_oracle.py); every expectation is computed before the GPU is touched; no env
is exempt from anything (tests/test_mates_queries.py: no fatal flag, no FLAME_QUEUE_RANGE under any mask).  rollout_jobs and expand
get their company from their LISTS: the handle holds each of the 112 states once and the source list is the composition, so that job
group g is wavefront g of the batch.

That the net holds was shown once on an MI355X, as in test_tile_mates.py, with libraries built from one-line changes that move rows
or columns inside a kernel's own LDS array (GPU tests failing here / in test_tile_mates.py / in the rest of the GPU suite, which was
run without test_gpu_chain, test_bench_cli, test_gpu_full_rows and test_dist_gloo):
  step_mixed's restart from the snapshot writes column ec_u ^ 1                  2 /  0 / 11   (the rest: test_step_mixed.py)
  its end-of-tick restart writes column ec_u ^ 1                                 2 /  0 /  6   (test_step_mixed.py)
  the park rows behind RP_ROWS moved into the claim rows (ROW_CLAIMS + 8)        4 /  0 / 42
  FC_STAGE_ROW 12 rows down                                                      2 /  0 / 12
  expand's gather lays a job over column col ^ 1                                 2 /  0 / 31
  claims() reads the map of column el ^ 1                                       18 / 18 / 93   (all here but the six restart tests,
                                                                                                whose family holds no select victim)"""
import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import edge_queries as EQ
from tests import mates_queries as MQ
from tests import rollout_oracle as RO
from tests import tile_mates as TM
from tests.range_model import RESET_AT_END, RESET_AT_START
from tests.test_tile_mates import _check

pytestmark = pytest.mark.gpu
T = TM.TICKS
FUSED_TICKS = 4          # the SimpleAgent runs write the fused views on the decisive ticks 0 .. 3


@pytest.fixture(scope="module")
def mates(oracle):
    return MQ.mates(oracle)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to("cuda")   # (the expectations are kept read-only)


def _same(M, what, got, want, env_axis=0, first=0):
    """a device tensor or an array against the expectation, byte for byte; a difference is named by its env and its wavefront"""
    import torch
    want = np.ascontiguousarray(want)
    if hasattr(got, "is_cuda") and got.is_cuda and tuple(got.shape) == want.shape and got.element_size() == want.dtype.itemsize:
        w = _dev(want.view(np.int32) if want.dtype == np.uint32 else want)
        if torch.equal(got.view(w.dtype), w):
            return
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    if got.dtype != want.dtype:
        assert got.dtype.itemsize == want.dtype.itemsize, (what, got.dtype, want.dtype)
        got = got.view(want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} values differ in {len(set(bad[:, env_axis].tolist()))} envs, first at {bad[0].tolist()}: got "
                           f"{got[tuple(bad[0])]}, want {want[tuple(bad[0])]}; {M.name_of_env(first + bad[0][env_axis])}")


def _fused(form, n):
    """sentinel-filled outputs of a fused observation and the keywords that ask for it: (out, attrs, env_attrs, keywords)"""
    import torch
    if form == "none":
        return None, None, None, {}
    e_attrs = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    if form == "fogged_codes":
        out = torch.full((n, 4, 5, 11, 11), 0xEE, dtype=torch.uint8, device="cuda")
        attrs = torch.full((n, 4, 12), -7, dtype=torch.int32, device="cuda")
        kw = dict(codes=out, view_radius=MQ.VIEW_RADIUS, viewer_attrs=attrs, env_attrs=e_attrs)
    else:
        out = torch.full((n, 4, 16, 11, 11), -7.0, dtype=torch.float16, device="cuda")
        attrs = torch.full((n, 4, 8), -7, dtype=torch.int32, device="cuda")
        kw = dict(planes=out, per_agent=True, agent_attrs=attrs, env_attrs=e_attrs)
    torch.cuda.synchronize()   # the sentinels are in place before the handle's stream writes
    return out, attrs, e_attrs, kw


def _same_obs(M, what, outs, want, rows=None, first=0):
    out, attrs, e_attrs = outs
    planes, want_attrs, env2 = want
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    _same(M, f"{what}: planes", out, pick(planes), first=first)
    _same(M, f"{what}: attrs", attrs, pick(want_attrs), first=first)
    _same(M, f"{what}: env_attrs", e_attrs[:, :2].contiguous(), pick(env2), first=first)


def _ranges(n):
    """two ranges cut at a tile boundary: the second has block0 != 0 and ends in the short tile"""
    cut = n // 3 - (n // 3) % 16
    return (0, cut), (cut, n - cut)


# ---------------------------------------------------------------------------------------------------------------- a. step_mixed, scripts
@pytest.mark.parametrize("form", ["none", "fogged_codes", "per_agent_f16"])
def test_step_mixed_plays_the_scripts(hip_lib, mates, form):
    """MODE_RAW, mask 0, two ranges: all 16 ticks, state and sticky flags are each env's actor's solo trace; the fused fogged codes
    (radius 4, viewer_attrs) and the per-agent float16 planes after every tick are the oracles' of that state"""
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    M, n = mates, mates.n
    want = {"none": lambda t: None, "fogged_codes": M.trace_views, "per_agent_f16": M.trace_planes}[form]
    for t in range(T):
        want(t)
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(M.start)
        env.sync()
        out, attrs, e_attrs, kw = _fused(form, n)
        for t in range(T):
            mv = _dev(M.script[t])
            for first, count in _ranges(n):
                env.step_mixed(first, count, mv, 0, MQ.SEED, t, None, **kw)
            env.sync()
            _check(M.stage, M.fam, 16, M.who, t, env.get_state(), env.status()["ubflags"], f"step_mixed, {form}: ")
            if form != "none":
                _same_obs(M, f"step_mixed, {form}, tick {t}", (out, attrs, e_attrs), want(t), rows=M.who)
        assert not env.policy_memory().any()


# ---------------------------------------------------------------------------------------------------------------- b. step_mixed, SimpleAgents
@pytest.mark.parametrize("mask", MQ.MASKS, ids=["mask_0110", "mask_1111"])
def test_step_mixed_simple_agents(hip_lib, mates, mask):
    """MODE_ENV without reset: the policy's maps lie over the rows the previous tick's frames used and under the export's staging rows.
    Everything the API can read, policy_memory() included, against the model after every call; the fused fogged codes on ticks 0 .. 3"""
    from pomcpp_amd.batch import MODE_ENV, RESET_OFF, BatchEnvironment
    M, n = mates, mates.n
    frames = M.frames(mask)
    views = [M.views(frames[t].readable()["state"]) for t in range(FUSED_TICKS)]
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_OFF) as env:
        env.make_game(M.start)
        env.sync()
        out, attrs, e_attrs, kw = _fused("fogged_codes", n)
        for t in range(T):
            mv = _dev(M.script[t])
            for first, count in _ranges(n):
                env.step_mixed(first, count, mv, mask, MQ.SEED, t, None, **(kw if t < FUSED_TICKS else {}))
            env.sync()
            frames[t].same_as(env, f"mask {mask:#x}, tick {t}")
            if t < FUSED_TICKS:
                _same_obs(M, f"mask {mask:#x}, tick {t}, fused fogged codes", (out, attrs, e_attrs), views[t])


# ---------------------------------------------------------------------------------------------------------------- c. step_mixed, restarts
RESTARTS = {"at_start": (RESET_AT_START, False), "at_start_fresh": (RESET_AT_START, True), "at_end": (RESET_AT_END, False)}


@pytest.mark.parametrize("mask", [0, 0xF], ids=["scripts", "mask_1111"])
@pytest.mark.parametrize("mode", list(RESTARTS))
def test_step_mixed_restarts_beside_detonating_mates(hip_lib, mates, mode, mask):
    """the kernel's three restart paths (the snapshot, a fresh board, the end of the tick), cap ENV_CAP: 0, 1, 2, 15 and 16 columns of a
    wavefront are rewritten beside mates whose chains go off on that tick and the next.  After every tick: states, statuses, episodes,
    terminal records, last_results, counters, and the agents' memory, wiped where an env restarted"""
    from pomcpp_amd.batch import MODE_ENV, BatchEnvironment
    M = mates
    frames = M.restarts(RESTARTS[mode], mask)
    lo, cnt = M.family("restart")
    auto_reset, fresh = RESTARTS[mode]
    with BatchEnvironment(cnt, mode=MODE_ENV, auto_reset=auto_reset, max_steps=TM.ENV_CAP, fresh_boards=fresh, board_seed=MQ.BOARD_SEED) as env:
        env.make_game(M.start[lo:lo + cnt])
        env.sync()
        for t, (frame, _) in enumerate(frames):
            env.step_mixed(0, cnt, _dev(M.restart_moves(t)), mask, MQ.SEED, t)
            env.sync()
            frame.same_as(env, f"{mode}, mask {mask:#x}, tick {t}")


# ---------------------------------------------------------------------------------------------------------------- d. the step kernels' fogged export
def test_step_kernels_fogged_export(hip_lib, mates):
    """step_device_observe(dtype="codes", view_radius=4) and step_device_range with the views, 16 ticks under the scripts: what
    test_mates_gpu_tape_observe_and_range checks for the unfogged forms"""
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    M, n = mates, mates.n
    for t in range(T):
        M.trace_views(t)
    moves = [_dev(M.script[t]) for t in range(T)]
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(M.start)
        for t in range(T):
            outs = env.step_device_observe(moves[t], dtype="codes", view_radius=MQ.VIEW_RADIUS)
            env.sync()
            _check(M.stage, M.fam, 16, M.who, t, env.get_state(), env.status()["ubflags"], "step_device_observe, fogged codes: ")
            _same_obs(M, f"step_device_observe, fogged codes, tick {t}", outs, M.trace_views(t), rows=M.who)
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(M.start)
        env.sync()
        out, attrs, e_attrs, kw = _fused("fogged_codes", n)
        for t in range(T):
            for first, count in _ranges(n):
                env.step_device_range(first, count, moves[t], None, **kw)
            env.sync()
            _check(M.stage, M.fam, 16, M.who, t, env.get_state(), env.status()["ubflags"], "step_device_range, fogged codes: ")
            _same_obs(M, f"step_device_range, fogged codes, tick {t}", (out, attrs, e_attrs), M.trace_views(t), rows=M.who)


# ---------------------------------------------------------------------------------------------------------------- e. the search calls on the batch
def _asked(M, t0, ask):
    """the batch at tick t0 — the first tick a kernel plays on it is the actors' decisive one — on a MODE_ENV handle without reset:
    ask(env, q, the moves on the device); the batch is left byte for byte and no flag is raised on it"""
    from pomcpp_amd.batch import MODE_ENV, RESET_OFF, BatchEnvironment
    q = M.at(t0)
    with BatchEnvironment(q.n, mode=MODE_ENV, auto_reset=RESET_OFF) as env:
        env.make_game(q.placed)
        ask(env, q, _dev(q.placed_moves))
        assert env.get_state().tobytes() == q.placed.tobytes(), "a call changed the batch"
        assert not env.status()["ubflags"].any()


@pytest.mark.parametrize("t0", MQ.T0S)
def test_forecast(hip_lib, mates, t0):
    """horizon 32 with the moves, and its prefixes 1 and 7 (their flags a run of their own)"""
    M = mates
    for h in (EQ.FORECAST_K,) + EQ.FORECAST_PREFIXES:
        M.at(t0).forecast(True, h)

    def ask(env, q, mv):
        for h in (EQ.FORECAST_K,) + EQ.FORECAST_PREFIXES:
            got = env.forecast(h, moves=mv, ubflags=True)
            for name, want in zip(("flame_tick", "agent_tick", "ubflags"), q.forecast(True, h)):
                _same(M, f"forecast, horizon {h}: {name}", got[name], want[q.order])
    _asked(M, t0, ask)


@pytest.mark.parametrize("t0", MQ.T0S)
def test_move_safety(hip_lib, mates, t0):
    """horizon 10, all agents, the others standing still"""
    M = mates
    M.at(t0).move_safety(False)

    def ask(env, q, mv):
        got = env.move_safety(MQ.SAFETY_K)
        for name, want in zip(("death_tick", "escape_tick"), q.move_safety(False)):
            _same(M, f"move_safety: {name}", got[name], want[q.order])
    _asked(M, t0, ask)


@pytest.mark.parametrize("t0", MQ.T0S)
def test_rollout(hip_lib, mates, t0):
    """DIST_STRESS after the moves, 24 ticks, 2 samples"""
    M = mates
    M.at(t0).rollout(RO.DIST_STRESS, True)

    def ask(env, q, mv):
        got = env.rollout(MQ.ROLLOUT_K, MQ.ROLLOUT_R, MQ.SEED, RO.DIST_STRESS, moves=mv)
        _same(M, "rollout, DIST_STRESS after the moves", got, q.rollout(RO.DIST_STRESS, True), env_axis=1)
    _asked(M, t0, ask)


@pytest.mark.parametrize("t0", MQ.T0S)
def test_rollout_with_simple_agents(hip_lib, mates, t0):
    """SimpleAgents in seats 1 and 3, 12 ticks: from fresh agents, and from the memory policy_simple leaves on the handle (what one
    step_simple tick leaves on a twin: no env restarts), so that the dwords parked behind the tile are not zero"""
    M = mates
    M.memory(t0), M.rollout_policy(t0, True), M.rollout_policy(t0, False)

    def ask(env, q, mv):
        got = env.rollout(MQ.POLICY_K, MQ.POLICY_R, MQ.SEED, RO.DIST_RANDOM, simple=MQ.POLICY_MASK, fresh_agents=True)
        _same(M, "rollout, SimpleAgents, fresh", got, M.rollout_policy(t0, True), env_axis=1)
        moves = env.policy_simple(MQ.SEED, want_moves=True)
        assert np.array_equal(moves, M.memory(t0)[1]) and np.array_equal(env.policy_memory(), M.memory(t0)[0])
        got = env.rollout(MQ.POLICY_K, MQ.POLICY_R, MQ.SEED, RO.DIST_RANDOM, simple=MQ.POLICY_MASK)
        _same(M, "rollout, SimpleAgents, from the handle's memory", got, M.rollout_policy(t0, False), env_axis=1)
        assert np.array_equal(env.policy_memory(), M.memory(t0)[0])
    _asked(M, t0, ask)


# ---------------------------------------------------------------------------------------------------------------- f. rollout_jobs
@pytest.mark.parametrize("t0", MQ.T0S)
def test_rollout_jobs_gathers_the_company(hip_lib, mates, t0):
    """the handle holds the 112 states once; the source list is the composition, then 11 entries that are no job, then the 112 envs in
    order (groups that are loaded as a tile, not gathered): 24 ticks, 2 samples, DIST_STRESS after the jobs' moves, agent 2 a SimpleAgent"""
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    M, h = mates, mates.once_each(t0)
    src, mv, want = M.jobs(t0)
    with BatchEnvironment(h.n, mode=MODE_RAW) as env:
        env.make_game(h.placed)
        got = env.rollout_jobs(_dev(src), MQ.ROLLOUT_K, MQ.ROLLOUT_R, MQ.SEED, RO.DIST_STRESS, moves=_dev(mv), simple=MQ.JOBS_SIMPLE,
                               first=MQ.JOBS_FIRST, fresh_agents=True)
        got = got.cpu().numpy().view(np.uint32)
        assert env.get_state().tobytes() == h.placed.tobytes(), "the call changed the batch"
    bad = np.argwhere(got != want)
    if bad.size:
        r, j = bad[0].tolist()
        where = M.name_of_env(j) if j < M.n else f"job {j} of the tail (source {src[j]})"
        raise AssertionError(f"{len(bad)} words differ in {len(set(bad[:, 1].tolist()))} jobs, first sample {r}: got {got[r, j]:#x}, want {want[r, j]:#x}; {where}")


# ---------------------------------------------------------------------------------------------------------------- g. expand
@pytest.mark.parametrize("mode", [0, 1], ids=["raw", "env"])
def test_expand_lays_the_company_over_the_slots(hip_lib, mates, mode):
    """the 112 states and 3,381 slots behind them: slot j becomes the child of env who[j] under the script's row 0 — the job columns of
    a destination tile are a wavefront of the composition —, then the identity list plays row 1 on every slot.  Words, children,
    statuses and the fused code planes of the children are the checkers'; the sources are untouched.  MODE_RAW: the children are the
    solo traces at ticks 0 and 1"""
    import torch
    from pomcpp_amd.batch import RESET_OFF, BatchEnvironment
    M, A = mates, mates.actors
    calls = M.expand(mode)
    ob = EQ.observe_oracle()
    obs = []
    for _, _, both, _, _ in calls:
        _, attrs, env2 = ob.observe(both[A:])
        obs.append((ob.observe_codes(both[A:]), attrs, env2))
    n = A + M.n
    with BatchEnvironment(n, mode=mode, auto_reset=RESET_OFF) as env:
        env.make_game(np.concatenate([M.distinct(0)[0], np.zeros(M.n, dtype=STATE_DTYPE)]))
        for t, (src, mv, both, status, want_words) in enumerate(calls):
            codes = torch.full((n, 5, 11, 11), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            words, a_attrs, e_attrs = env.expand(_dev(src), _dev(mv), first=A, codes=codes)
            words = words.cpu().numpy().view(np.uint32)
            got, st = env.get_state(), env.status()
            bad = np.nonzero(words != want_words)[0]
            assert bad.size == 0, f"call {t}: {len(bad)} words differ, first got {words[bad[0]]:#x}, want {want_words[bad[0]]:#x}; {M.name_of_env(bad[0])}"
            assert got[:A].tobytes() == both[:A].tobytes(), f"call {t}: a source changed"
            if mode == 0:
                _check(M.stage, M.fam, 16, M.who, t, got[A:], st["ubflags"][A:], f"expand, call {t}: ")
            _same(M, f"call {t}: children", got[A:].view(np.uint8).reshape(-1, 1004), both[A:].view(np.uint8).reshape(-1, 1004))
            for k in ("done", "winner", "draw", "ubflags"):
                _same(M, f"call {t}: status {k}", np.asarray(st[k][A:]).astype(status[k].dtype), status[k][A:])
            _same_obs(M, f"call {t}: fused codes", (codes[A:], a_attrs[A:].contiguous(), e_attrs[A:]), obs[t])
            assert bool((codes[:A] == 0xEE).all()), f"call {t}: observation rows of the sources were written"
