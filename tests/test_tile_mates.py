"""An env's tick must not depend on the envs that share its wavefront (actors and compositions: tests/tile_mates.py).

The kernels share a great deal across the 16 (32, 64) envs of a wavefront, most of it resting on "the wavefront runs in lock-step":
loop B's per-cell counters [env][124 bytes] lie over the explosion frames [row][EPW] (pom_tile.h ROW_CLAIMS == ROW_STACK), a
restarting env's column is rewritten by the whole wavefront, the policy's maps and the observation's staging area lie over the tick's
scratch rows, and the bomb / blast / bounce loops run as long as the worst mate needs.  Every other parity test compares an env with
the oracle in whatever company it happens to keep; here the company is chosen.

CPU (unmarked): every actor, every tick, through the one-lane and the four-lane host build of the device tick against the oracle,
byte for byte, zero exemptions; the instrumented host builds (tests/emul/pom_emul_probe.h) prove that the actors reach what they are
for; the oracle is pinned on the actors against the compiled reference (tests/golden/tile_mates.npz); the compositions are recounted
from their arrays.  GPU: the expected State of an env under explicit moves is its actor's SOLO oracle trace, whatever its place.

Measured with the instrumented builds: the deepest frame index 20 queued bombs reach is 18 = POM_STACK_DEPTH - 3.  A frame is pushed
when a blast meets a bomb, and the bomb that starts a chain is not met by any: 20 bombs push 19 frames, rows 0 .. 18.  Rows 19 and 20
of the stack cannot be written by a state upload accepts.  Overlay pairs (d, A) that remain after the pad bytes and B == A are
skipped: 276 of 304 (EPW 16), 570 of 608 (EPW 32), 1158 of 1216 (EPW 64), each in both phases.

That the net holds was shown once on an MI355X with libraries built from one-line changes that only alter which bytes of the
wavefront's own LDS tile are used (GPU tests failing here / in test_record_edges.py / in test_gpu_parity.py):
  loop_b_todo writes set_frame(0, a frame) of its own column between counting and reading             14 /  0 / 1
  claim_map() stride 124 -> 120                                                                         0 /  0 / 0   (behaviour-
      preserving: test_counts_too_high_change_nothing)  replaced by: claims() reads the map of column el ^ 1   14 /  0 / 2
  the restart from the snapshot writes column ec_u ^ 1                                                 10 /  1 / 2
  the fresh board of a restart is drawn into column ec_u ^ 1                                            4 /  0 / 0
  the end-of-tick restart writes column ec_u ^ 1                                                        1 /  1 / 0
  bdest() / put_bdest() of columns el and el ^ 1 share their rows                                      13 /  0 / 2

The GPU part here runs pom_step_kernel only.  The kernels that embed the same tick in an LDS array of their own — the mixed step, the
rollouts, forecast, move_safety, expand, the fogged export — meet this module's batch in tests/test_gpu_mates_queries.py."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE, Item
from tests import tile_mates as TM
from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE, UB_REVERT_LOOP
from tests.test_emul import emul_bins  # noqa: F401  (the host builds of the device body)
from tests.test_record_edges import _hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tile_mates.npz")
T = TM.TICKS
PROBE_WORDS = 8 + TM.LAYOUT["stack_depth"]
P_MAXFRAME, P_MASK, P_NCLAIM, P_TODO_RAN, P_CLAIMED, P_REM0, P_HOPS, P_FRAMES = 0, 1, 2, 3, 4, 5, 6, 8
SHAPES = [(16, 4), (16, 1), (32, 1), (64, 1)]
OVERLAY_PAIRS = {16: 276, 32: 570, 64: 1158}


class Stage:
    def __init__(self, oracle):
        self.entries = TM.actors(oracle)
        self.cast = TM.Cast(self.entries)
        self.states, self.ubs = TM.solo_traces(oracle, self.entries)
        self.sticky = np.bitwise_or.accumulate(self.ubs, axis=1)


@pytest.fixture(scope="module")
def stage(oracle):
    return Stage(oracle)


def _run_probe(lib, e, quad, cap=None, add=0):
    """T ticks of one actor through a host build: states uint8[T, 1004], flags, the probe's counters int32[T, PROBE_WORDS]"""
    run = lib.pom_emul_run_probe
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    run.restype = C.c_int
    lib.pom_emul_probe_claims_cap.argtypes = [C.c_int, C.c_int]
    got, ubs = np.zeros((T, 1004), dtype=np.uint8), np.zeros(T, dtype=np.uint32)
    probe = np.zeros((T, PROBE_WORDS), dtype=np.int32)
    mv = np.ascontiguousarray(e.moves, dtype=np.int32)
    lib.pom_emul_probe_claims_cap(0x7FFFFFFF if cap is None else cap, add)
    try:
        assert run(e.start.ctypes.data, mv.ctypes.data, T, quad, got.ctypes.data, ubs.ctypes.data, probe.ctypes.data) == 0, \
            f"{e.name}: upload refuses the start state"
    finally:
        lib.pom_emul_probe_claims_cap(0x7FFFFFFF, 0)
    return got, ubs, probe


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_layout_is_what_the_overlay_family_was_built_for():
    assert TM.layout() == TM.LAYOUT, "layout changed: re-derive the overlay family"
    # the counters lie OVER the frames, an env's map is 124 bytes, and a frame's top byte is rem >> 5
    assert TM.LAYOUT["row_stack"] == TM.LAYOUT["row_claims"]
    for epw in (16, 32, 64):
        assert TM.alias(epw, 0, 0) == (0, 0) and TM.alias(epw, 1, 0) == ((4 * epw) // 124, (4 * epw) % 124)


def test_no_actor_raises_a_fatal_flag_and_every_tick_counts(stage):
    for e, ubs in zip(stage.entries, stage.ubs):
        assert not int(np.bitwise_or.reduce(ubs)) & (FATAL | UB_FLAME_QUEUE_RANGE), e.name
    kinds = {TM.kind(e.name) for e in stage.entries}
    assert kinds == {"deep_b", "deep_top", "select", "claims_full", "bounce", "quiet", "edge"}
    assert int(np.bitwise_or.reduce(stage.ubs[stage.cast.ix["edge_ub_lost_agent"]])) == 1  # LOST_AGENT travels along


@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_device_tick_body_matches_oracle_on_every_actor(emul_bins, stage, quad):  # noqa: F811
    """every tick of every actor, the record packed once and kept between ticks: all 1004 bytes and ubflags; the quad model's checks"""
    for i, e in enumerate(stage.entries):
        got, ubs, _ = _run_probe(emul_bins, e, quad)
        assert not (ubs & 0x40000000).any(), f"{e.name}: the quad model's checks failed"
        assert np.array_equal(ubs, stage.ubs[i]), f"{e.name}: ubflags {ubs.tolist()}, oracle {stage.ubs[i].tolist()}"
        bad = np.nonzero((got != stage.states[i]).any(axis=1))[0]
        assert bad.size == 0, f"{e.name} tick {bad[0]}: bytes {np.nonzero(got[bad[0]] != stage.states[i, bad[0]])[0][:12].tolist()} differ"


@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_deep_chains_write_every_frame_row_they_are_for(emul_bins, stage, quad):  # noqa: F811
    deepest, rows_b, rows_top = -1, 0, 0
    for i, e in enumerate(stage.entries):
        if not e.name.startswith("deep_"):
            continue
        depth = int(e.name.rsplit("_d", 1)[1])
        tick = 1 if ("push1" in e.name or "top1" in e.name) else 0
        _, _, pr = _run_probe(emul_bins, e, quad)
        p = pr[tick]
        assert p[P_MAXFRAME] == depth - 1 and p[P_MASK] == (1 << depth) - 1, (e.name, p[:8].tolist())
        assert (pr[:tick, P_MAXFRAME] == -1).all(), e.name  # nothing before its tick
        bombs = stage.states[i].view(STATE_DTYPE)["bombs_count"][:, 0]
        assert int(bombs[tick]) == 20 - (depth + 1) and (tick == 0 or int(bombs[0]) == 20), (e.name, bombs.tolist())
        frames = p[P_FRAMES:P_FRAMES + depth].astype(np.uint32)
        if e.name.startswith("deep_b"):
            # set off inside loop B: loop_b_todo ran in that tick, the chain's first frame names a queue offset, and every frame's top
            # byte (rem >> 5) is 0: below the 2 that selects a victim's K
            assert p[P_TODO_RAN] == 1 and 0 <= p[P_REM0] < 20, (e.name, p[:8].tolist())
            assert ((frames >> 24) == 0).all(), (e.name, [hex(f) for f in frames])
            rows_b |= int(p[P_MASK])
        else:
            assert p[P_REM0] == 62, (e.name, p[:8].tolist())  # REM_TOP: TickBombs, after loop B
            assert ((frames >> 24) <= 1).all(), e.name
            rows_top |= int(p[P_MASK])
        deepest = max(deepest, int(p[P_MAXFRAME]))
    # 20 queued bombs push 19 frames (the bomb that starts the chain is met by no blast): rows 0 .. 18 = POM_STACK_DEPTH - 3
    assert deepest == 18 == TM.LAYOUT["stack_depth"] - 3 == TM.MAX_DEPTH - 1
    assert rows_b == rows_top == (1 << 19) - 1
    for trig in ("deep_b_rest", "deep_b_push", "deep_b_push1", "deep_top"):
        i = stage.cast.ix[f"{trig}_d19"]
        tick = 1 if trig.endswith("1") else 0
        assert int(stage.states[i].view(STATE_DTYPE)["bombs_count"][tick, 0]) == 0 and not stage.ubs[i].any(), trig  # 20 -> 0 in one tick


@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_select_victims_need_their_counter(emul_bins, stage, quad):  # noqa: F811
    """K (queue offset 0, resting, its cell shows BOMB) is in loop_b_todo's answer only through the counter of its cell; with the
    counter read as at most 1 the tick gives ANOTHER state: the construction is decisive"""
    n = 0
    for i, e in enumerate(stage.entries):
        if not e.name.startswith("select") or e.name == "select_pairs20":
            continue
        tick = 1 if e.name.startswith("select1") else 0
        s0 = e.start
        k = int(s0["bombs_queue"][0, int(s0["bombs_index"][0])])
        kx, ky = k & 0xF, (k >> 4) & 0xF
        assert (k >> 20) & 0xF == 0 and int(s0["board"][0, ky, kx]) == Item.BOMB, e.name
        _, _, pr = _run_probe(emul_bins, e, quad)
        assert pr[tick, P_TODO_RAN] == 1 and pr[tick, P_CLAIMED] & 1, (e.name, pr[tick, :8].tolist())
        after = stage.states[i, tick].view(STATE_DTYPE)[0]
        j = int(after["bombs_queue"][(int(s0["bombs_index"][0]) + 1) % 20])
        assert (j >> 20) & 0xF == 0 and (j & 0xFF) != (k & 0xFF) and abs((j & 0xF) - kx) + abs(((j >> 4) & 0xF) - ky) == 1, e.name  # J stopped next to K
        blind, _, _ = _run_probe(emul_bins, e, quad, cap=1)
        assert np.array_equal(blind[:tick], stage.states[i, :tick]) and not np.array_equal(blind[tick], stage.states[i, tick]), \
            f"{e.name}: a counter read as 1 does not change the result"
        n += 1
    assert n == 2 * len(TM.SELECT_CELLS) + 2
    e = stage.entries[stage.cast.ix["select_pairs20"]]
    _, _, pr = _run_probe(emul_bins, e, quad)
    ks = sum(1 << o for o in range(20) if (int(e.start["bombs_queue"][0, o]) >> 20) & 0xF == 0)
    assert bin(ks).count("1") == 10 and pr[0, P_CLAIMED] & ks == ks, hex(pr[0, P_CLAIMED])
    blind, _, _ = _run_probe(emul_bins, e, quad, cap=1)
    assert not np.array_equal(blind[0], stage.states[stage.cast.ix["select_pairs20"], 0])


@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_counts_too_high_change_nothing(emul_bins, stage, quad):  # noqa: F811
    """the other direction: a counter that reads too HIGH only selects bombs whose turn does nothing (loop_b_todo's set may be too
    large, never too small).  This is why claim maps that merely overlap (claim_map() with a stride of 120: counts of a neighbour's
    cells 0 .. 3 land on cells 120 .. 123) give the same results on the device: a wavefront in lock-step clears all its maps before
    it counts in any, so an overlap only ever adds"""
    for i, e in enumerate(stage.entries):
        got, ubs, pr = _run_probe(emul_bins, e, quad, add=2)
        assert np.array_equal(got, stage.states[i]) and np.array_equal(ubs, stage.ubs[i]), e.name
        ran = pr[:, P_TODO_RAN] == 1
        n_bombs = np.concatenate([[int(e.start["bombs_count"][0])], stage.states[i].view(STATE_DTYPE)["bombs_count"][:-1, 0]])
        assert all(int(pr[t, P_CLAIMED]) == (1 << int(n_bombs[t])) - 1 for t in np.nonzero(ran)[0]), e.name  # every bomb selected


def test_claims_full_touches_every_dword_of_the_map(emul_bins, stage):  # noqa: F811
    e = stage.entries[stage.cast.ix["claims_full"]]
    dx, dy = {1: 0, 2: 0, 3: -1, 4: 1}, {1: -1, 2: 1, 3: 0, 4: 0}
    dwords = set()
    for o in range(20):
        b = int(e.start["bombs_queue"][0, o])
        x, y, d = b & 0xF, (b >> 4) & 0xF, (b >> 20) & 0xF
        assert d in dx and 0 <= x + dx[d] <= 10 and 0 <= y + dy[d] <= 10
        dwords |= {(y * 11 + x) // 4, ((y + dy[d]) * 11 + x + dx[d]) // 4}
    assert dwords == set(range(31))
    for quad in (0, 1):
        _, _, pr = _run_probe(emul_bins, e, quad)
        assert pr[0, P_TODO_RAN] == 1 and pr[0, P_NCLAIM] == 40, pr[0, :8].tolist()


@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_bounce_chains_reach_their_hops_from_loop_b(emul_bins, stage, quad):  # noqa: F811
    for h in sorted(TM.BOUNCES):
        i = stage.cast.ix[f"bounce_{h}"]
        _, ubs, pr = _run_probe(emul_bins, stage.entries[i], quad)
        assert pr[0, P_TODO_RAN] == 1 and pr[0, P_HOPS] == h, (h, pr[0, :8].tolist())
        assert not int(np.bitwise_or.reduce(ubs)) & UB_REVERT_LOOP
    assert max(TM.BOUNCES) == 7


def test_oracle_reproduces_the_reference_on_the_actors(oracle, stage):
    """every tick the compiled reference played of every actor (tests/golden/gen_tile_mates.py): the oracle's state hash after it,
    and the full states at the checkpoints"""
    g = np.load(GOLDEN)
    assert [e.name for e in stage.entries] == list(g["names"]), "the actors changed: regenerate tests/golden/tile_mates.npz"
    ck = {(int(a), int(t)): g["ck_state"][k] for k, (a, t) in enumerate(zip(g["ck_entry"], g["ck_tick"]))}
    assert g["hashes"].shape == (len(stage.entries), T)  # zero ticks exempt: the reference played them all
    for i, e in enumerate(stage.entries):
        assert e.start.tobytes() == g["start"][i].tobytes(), e.name
        assert np.array_equal(e.moves, g["moves"][i]), e.name
        for t in range(T):
            assert _hash(stage.states[i, t].tobytes()) == int(g["hashes"][i, t]), f"{e.name}: the oracle leaves the reference at tick {t}"
            if (i, t + 1) in ck:
                assert stage.states[i, t].tobytes() == ck[(i, t + 1)].tobytes(), f"{e.name}: checkpoint after tick {t}"
    assert len(ck) >= 3 * len(stage.entries)


def _deep_b_info(name):
    """(frames, tick it goes off) of a deep_b actor, else None"""
    if not name.startswith("deep_b"):
        return None
    return int(name.rsplit("_d", 1)[1]), int("push1" in name)


@pytest.mark.parametrize("epw", [16, 32, 64])
def test_compositions_cover_what_they_claim(stage, epw):
    """recounted from the arrays alone"""
    cast, names = stage.cast, stage.cast.names
    # overlay: every (d, A) left by the arithmetic, in both phases
    who, _ = TM.overlay(cast, epw)
    assert who.size % epw == 0
    found = set()
    for w in range(who.size // epw):
        cols = [names[i] for i in who[w * epw:(w + 1) * epw]]
        for a, nm in enumerate(cols):
            info = _deep_b_info(nm)
            if info is None:
                continue
            frames, phase = info
            for d in range(frames):
                b, byte = TM.alias(epw, d, a)
                if b < epw and cols[b] == f"select{phase or ''}_c{byte + 3}":
                    found.add((d, a, phase))
    expect = {(d, a, ph) for (d, a, b, c) in TM.overlay_pairs(epw) for ph in (0, 1)}
    assert expect <= found
    assert len(TM.overlay_pairs(epw)) == OVERLAY_PAIRS[epw] and OVERLAY_PAIRS[epw] > 0.9 * 19 * epw
    assert {d for d, _, _ in expect} == set(range(19)) and {a for _, a, _ in expect} == set(range(epw))
    # pairs
    who = TM.pairs(cast, epw)
    seen, at_col = set(), set()
    for w in range(who.size // epw):
        kinds = [cast.kinds[i] for i in who[w * epw:(w + 1) * epw]]
        present = set(kinds)
        seen |= {(a, v) for a in present for v in present}
        if present & {"deep_b", "claims_full"}:
            for c, k in enumerate(kinds):
                others = set(kinds[:c] + kinds[c + 1:])
                if others & {"deep_b", "claims_full"}:
                    at_col.add((k, c))
    assert {(a, v) for a in TM.AGGRESSORS for v in TM.VICTIMS} <= seen
    assert {(v, c) for v in TM.VICTIMS for c in range(epw)} <= at_col
    # crowd
    for tail in {16: (5,), 32: (5, 21), 64: (1, 17, 33)}[epw]:
        who = TM.crowd(cast, epw, tail)
        assert who.size % epw == tail and who.size % 16 != 0
        for heavy in (f"deep_b_rest_d{TM.MAX_DEPTH}", "claims_full", f"deep_top_d{TM.MAX_DEPTH}"):
            counts = [int((who[w * epw:(w + 1) * epw] == cast.ix[heavy]).sum()) for w in range(who.size // epw)]
            assert {0, 1, 2, epw - 1, epw} <= set(counts), (heavy, counts)
    # restart: how many envs of a wavefront finish on tick 0, and where they sit
    who = TM.restart(cast, epw)
    late = cast.ix["quiet_late_1"]
    counts, single = set(), set()
    for w in range(who.size // epw):
        cols = np.nonzero(who[w * epw:(w + 1) * epw] == late)[0]
        mates = {names[i] for i in who[w * epw:(w + 1) * epw]} - {"quiet_late_1"}
        counts.add(cols.size)
        if cols.size == 1:
            single.add(int(cols[0]))
        if 0 < cols.size < epw:
            assert any(m.startswith("deep_b") for m in mates), w
    assert {0, 1, 2, epw - 1, epw} <= counts and {0, epw // 2, epw - 1} <= single
    both = {_deep_b_info(names[i])[1] for i in who if _deep_b_info(names[i])}
    assert both == {0, 1}  # mates that go off on the tick of the restart and on the tick after


# ---------------------------------------------------------------------------------------------------------------- GPU
def _families(cast, epw):
    out = [("overlay", TM.overlay(cast, epw)[0]), ("pairs", TM.pairs(cast, epw)), ("restart", TM.restart(cast, epw))]
    out += [(f"crowd_tail{tail}", TM.crowd(cast, epw, tail)) for tail in {16: (5,), 32: (5, 21), 64: (1, 17, 33)}[epw]]
    return out


def _whole(cast, epw=16):
    """every family of the shape in one batch (each a whole number of wavefronts; the ragged crowd last): names and actors"""
    fams = _families(cast, epw)
    fams.sort(key=lambda f: f[1].size % epw != 0)
    assert all(f[1].size % epw == 0 for f in fams[:-1])
    who = np.concatenate([f[1] for f in fams[:4]])
    fam = sum(([f[0]] * f[1].size for f in fams[:4]), [])
    return fam, who


def _check(stage, fam, epw, who, t, got_states, got_ubs, what=""):
    """all 1004 bytes and the ubflags of every env against its actor's solo trace after tick t"""
    n = who.size
    g = got_states.view(np.uint8).reshape(n, 1004)
    w = stage.states[who, t]
    bad = np.nonzero((g != w).any(axis=1) | (np.asarray(got_ubs, dtype=np.uint32) != stage.sticky[who, t]))[0]
    if bad.size:
        k = int(bad[0])
        mates = [stage.cast.names[i] for i in who[k - k % epw:k - k % epw + epw]]
        raise AssertionError(
            f"{what}{fam[k] if isinstance(fam, list) else fam}: env {k} (wavefront {k // epw}, column {k % epw}) actor {stage.cast.names[who[k]]} tick {t}: "
            f"bytes {np.nonzero(g[k] != w[k])[0][:12].tolist()} differ, ubflags {int(got_ubs[k]):#x} want {int(stage.sticky[who[k], t]):#x}; "
            f"{bad.size} envs differ in all; its wavefront: {mates}")


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", SHAPES)
def test_mates_gpu_raw_step_every_tick(hip_lib, stage, epw, lpe):
    """RAW mode, env.step(moves): every family of the shape, every env, every tick"""
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    for fam, who in _families(stage.cast, epw):
        start, moves = TM.batch(stage.entries, who)
        with BatchEnvironment(who.size, mode=MODE_RAW, envs_per_wave=epw, lanes_per_env=lpe) as env:
            assert env.launch_shape()[:2] == (epw, lpe)
            env.make_game(start)
            for t in range(T):
                env.step(moves[t])
                _check(stage, fam, epw, who, t, env.get_state(), env.status()["ubflags"])


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", SHAPES)
def test_mates_gpu_env_step_finished_games_rest(hip_lib, oracle, stage, epw, lpe):
    """ENV mode without auto-reset, explicit moves: a finished game (quiet_one_alive after its first tick, quiet_all_dead, quiet_late_K
    with the cap at ENV_CAP) is not stepped again while its mates' chains go off; expected: each actor's solo run of oracle.env_step"""
    from pomcpp_amd.batch import MODE_ENV, BatchEnvironment
    A = len(stage.entries)
    states, ubs = np.zeros((A, T, 1004), dtype=np.uint8), np.zeros((A, T), dtype=np.uint32)
    done, winner = np.zeros(A, dtype=bool), np.zeros(A, dtype=np.int64)
    for i, e in enumerate(stage.entries):
        s, st = e.start.copy(), dict(done=0, winner=-1, draw=0)
        for t in range(T):
            if not (st["done"] or int(s["timeStep"][0]) >= TM.ENV_CAP):
                ubs[i, t] = oracle.env_step(s, e.moves[t], st)
            s["agents"]["pad"] = 0
            states[i, t] = np.frombuffer(s.tobytes(), dtype=np.uint8)
        done[i], winner[i] = bool(st["done"]) or int(s["timeStep"][0]) >= TM.ENV_CAP, st["winner"]
    sticky = np.bitwise_or.accumulate(ubs, axis=1)
    assert done[stage.cast.ix["quiet_one_alive"]] and done[stage.cast.ix["quiet_late_1"]] and done.all()  # the cap ends every game
    for fam, who in (("pairs", TM.pairs(stage.cast, epw)), ("restart", TM.restart(stage.cast, epw)),
                     ("crowd", TM.crowd(stage.cast, epw, {16: 5, 32: 21, 64: 33}[epw]))):
        start, moves = TM.batch(stage.entries, who)
        with BatchEnvironment(who.size, mode=MODE_ENV, auto_reset=False, max_steps=TM.ENV_CAP, envs_per_wave=epw, lanes_per_env=lpe) as env:
            env.make_game(start)
            for t in range(T):
                env.step(moves[t])
                g = env.get_state().view(np.uint8).reshape(who.size, 1004)
                st = env.status()
                bad = np.nonzero((g != states[who, t]).any(axis=1) | (st["ubflags"].astype(np.uint32) != sticky[who, t]))[0]
                assert bad.size == 0, (f"{fam}: env {bad[0]} (wavefront {bad[0] // epw}, column {bad[0] % epw}) actor "
                                       f"{stage.cast.names[who[bad[0]]]} tick {t}: bytes "
                                       f"{np.nonzero(g[bad[0]] != states[who[bad[0]], t])[0][:12].tolist()} differ; {bad.size} envs in all")
            assert st["done"].astype(bool).tolist() == done[who].tolist()
            assert st["winner"].tolist() == winner[who].tolist()


@pytest.mark.gpu
def test_mates_gpu_tape_observe_and_range(hip_lib, stage):
    """the default shape through every other way a tick is issued: the chained tape in pieces of 1, 2, 7 and the rest (no tile left
    behind), step + observation in one launch (uint8 planes and codes against oracle/pom_observe_oracle.py), the range call"""
    import importlib.util
    import torch
    from pomcpp_amd.batch import ISSUE_CHAIN, MODE_RAW, BatchEnvironment
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    ob = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ob)
    fam, who = _whole(stage.cast)
    n = who.size
    start, moves = TM.batch(stage.entries, who)
    dev_moves = torch.from_numpy(moves).to("cuda:0")
    with BatchEnvironment(n, mode=MODE_RAW, issue_mode=ISSUE_CHAIN) as env:
        env.make_game(start)
        t = 0
        for piece in (1, 2, 7, T - 10):
            env.step_device_many(dev_moves[t:t + piece].contiguous())
            env.sync()
            t += piece
            _check(stage, fam, 16, who, t - 1, env.get_state(), env.status()["ubflags"], "tape: ")
        stats = env.chain_stats()
        assert stats["tiles_recovered"] == 0 and stats["launches"] == 2 + 7 + T - 10, stats
    for dtype in ("uint8", "codes"):
        with BatchEnvironment(n, mode=MODE_RAW) as env:
            env.make_game(start)
            for t in range(T):
                out = env.step_device_observe(dev_moves[t].contiguous(), dtype=dtype)
                env.sync()
                states = env.get_state()
                _check(stage, fam, 16, who, t, states, env.status()["ubflags"], f"observe {dtype}: ")
                if dtype == "codes":
                    assert np.array_equal(out[0].cpu().numpy(), ob.observe_codes(states)), t
                else:
                    want, want_attrs, _ = ob.observe(states, per_agent=False, dtype=np.uint8)
                    assert np.array_equal(out[0].cpu().numpy(), want), t
                    assert np.array_equal(out[1].cpu().numpy(), want_attrs), t
    cut = (n // 3) - (n // 3) % 16
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(start)
        env.sync()
        for t in range(T):
            env.step_device_range(0, cut, dev_moves[t].contiguous())
            env.step_device_range(cut, n - cut, dev_moves[t].contiguous())
            env.sync()
            _check(stage, fam, 16, who, t, env.get_state(), env.status()["ubflags"], "range: ")


def _same(got, want, what):
    want = want.copy()
    want["agents"]["pad"] = 0
    g, w = got.view(np.uint8).reshape(-1, 1004), want.view(np.uint8).reshape(-1, 1004)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} envs differ, first env {bad[0]}, bytes {np.nonzero(g[bad[0]] != w[bad[0]])[0][:12].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("tpl", [4, 16])
@pytest.mark.parametrize("epw,lpe", SHAPES)
def test_mates_gpu_several_ticks_per_launch(hip_lib, oracle, stage, epw, lpe, tpl):
    """the tile stays in LDS between the ticks of a launch and the scratch rows are never re-initialised: the overlay and crowd
    batches as start states under the random move stream, against the oracle's run of the whole batch, after every launch"""
    from pomcpp_amd.batch import DIST_RANDOM, MODE_ENV, BatchEnvironment
    cast, seed = stage.cast, 23
    who = np.concatenate([TM.overlay(cast, epw)[0], TM.crowd(cast, epw, {16: 5, 32: 21, 64: 33}[epw])])
    start, _ = TM.batch(stage.entries, who)
    ref = start.copy()
    with BatchEnvironment(who.size, mode=MODE_ENV, auto_reset=True, max_steps=800, envs_per_wave=epw, lanes_per_env=lpe) as env:
        env.make_game(start)
        for k in range(32 // tpl):
            env.step_random(seed, DIST_RANDOM, ticks=tpl, ticks_per_launch=tpl)
            oracle.run_random(ref, start, tpl, seed, 0, k * tpl, DIST_RANDOM, 800)
            _same(env.get_state(), ref, f"epw {epw} tpl {tpl} after tick {(k + 1) * tpl - 1}")


RESTARTS = [("at_start", 16, 4), ("at_start", 16, 1), ("at_start", 32, 1), ("at_start", 64, 1), ("at_start_fresh", 16, 4),
            ("at_start_fresh", 16, 1), ("at_start_fresh", 32, 1), ("at_start_fresh", 64, 1), ("at_end", 16, 4)]  # (the end-of-tick reset is built for the quad shape only)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,epw,lpe", RESTARTS)
def test_mates_gpu_restarts_beside_detonating_mates(hip_lib, oracle, stage, mode, epw, lpe):
    """ENV mode, cap ENV_CAP: 0, 1, 2, EPW - 1, EPW envs of a wavefront finish on one tick and have their columns rewritten beside
    mates whose chains go off on that tick and the next; every tick against the oracle's run, every env restarts at least twice"""
    from pomcpp_amd.batch import (CNT_EPISODES, CNT_RESETS, CNT_STEPS, DIST_RANDOM, MODE_ENV, RESET_AT_END, RESET_AT_START,
                                  BatchEnvironment)
    cap, seed, bseed, ticks = TM.ENV_CAP, 5, 31, 3 * TM.ENV_CAP + 2
    who = TM.restart(stage.cast, epw)
    start, _ = TM.batch(stage.entries, who)
    n = who.size
    ref, eps = start.copy(), np.zeros(n, dtype=np.int32)
    finished = restarts = 0
    fresh, at_end = mode == "at_start_fresh", mode == "at_end"
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END if at_end else RESET_AT_START, max_steps=cap, fresh_boards=fresh,
                          board_seed=bseed, envs_per_wave=epw, lanes_per_env=lpe) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        env.make_game(start)
        for t in range(ticks):
            before = (ref["aliveAgents"] <= 1) | (ref["timeStep"] >= cap)
            restarts += int(before.sum())
            if fresh:
                oracle.run_random_fresh(ref, eps, 1, seed, bseed, 0, t, DIST_RANDOM, cap)
            else:
                oracle.run_random(ref, start, 1, seed, 0, t, DIST_RANDOM, cap)
                eps += before
            done = (ref["aliveAgents"] <= 1) | (ref["timeStep"] >= cap)
            finished += int(done.sum())
            env.step_random(seed, DIST_RANDOM, ticks=1)
            want = ref.copy()
            if at_end:
                want[done] = start[done]  # finished with this tick: already on the start state again
            _same(env.get_state(), want, f"{mode} tick {t}")
            if fresh:
                assert np.array_equal(env.episodes(), eps), t
            assert env.status()["done"].astype(bool).tolist() == ([False] * n if at_end else done.tolist()), t
        cnt = env.counters()
    assert eps.min() >= 2 and cnt[CNT_STEPS] == n * ticks and cnt[CNT_EPISODES] == finished
    assert cnt[CNT_RESETS] == (finished if at_end else restarts)


@pytest.mark.gpu
def test_mates_gpu_simple_policy(hip_lib, oracle, stage):
    """the fused policy kernel writes its danger map and cell sets over the rows the previous tick's frames used: overlay and crowd
    under four SimpleAgents against the oracle's policy and tick, states and agent memory after every call"""
    from pomcpp_amd.batch import MODE_ENV, BatchEnvironment
    cast, seed = stage.cast, 9
    who = np.concatenate([TM.overlay(cast, 16)[0], TM.crowd(cast, 16, 5)])
    start, _ = TM.batch(stage.entries, who)
    ref, mems = start.copy(), np.zeros((who.size, 4, 16), dtype=np.int32)
    with BatchEnvironment(who.size, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(start)
        tick = 0
        for k in (1, 1, 1, 2, 3, 8, 16):
            env.step_simple(seed, k)
            oracle.run_simple(ref, start, mems, k, seed, 0, tick, 800)
            tick += k
            _same(env.get_state(), ref, f"SimpleAgent after tick {tick - 1}")
            assert np.array_equal(env.policy_memory(), mems), tick
