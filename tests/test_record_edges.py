"""The tick at the limits of the packed record (pomcpp_amd/csrc/pom_packed.h), on the directed corpus of tests/edge_states.py.

CPU (unmarked): the oracle reproduces the compiled reference on every recorded tick of the corpus (tests/golden/edge_cases.npz);
the device tick body, built for the host one lane and four lanes per env (tests/emul), matches the oracle on every tick of every
entry, on a record packed once as the device keeps it; the packer accepts every field at its upload bound and refuses it one
step beyond.  GPU: the corpus in one ragged batch through every way a tick is issued, and the observations of its states.

Where the oracle raises POM_UB_FLAME_QUEUE_RANGE the record holds a flame timeLeft at -128 or flames.count at 255 (pom_state.h):
from that tick on only the flame queue's slots, flames.index and flames.count may differ from the oracle's state."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE, corpus
from tests.test_emul import emul_bins  # noqa: F401  (the host builds of the device body, built as test_emul.py builds them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "edge_cases.npz")
QUEUE_BYTES = slice(STATE_DTYPE.fields["flames_queue"][1], 1004)  # flames.queue, flames.index, flames.count: the tail of the State


def _hash(buf: bytes) -> int:
    import hashlib
    return int.from_bytes(hashlib.blake2b(buf, digest_size=8).digest(), "little")


@pytest.fixture(scope="module")
def edge_runs(oracle):
    """the corpus and the oracle's run of each entry: states after every tick (uint8[T, 1004]) and the tick's flags"""
    runs = []
    for e in corpus(oracle):
        s = e.start.copy()
        states, ubs = np.zeros((len(e.moves), 1004), dtype=np.uint8), np.zeros(len(e.moves), dtype=np.uint32)
        for t, mv in enumerate(e.moves):
            ubs[t] = oracle.step(s, mv)
            s["agents"]["pad"] = 0
            states[t] = np.frombuffer(s.tobytes(), dtype=np.uint8)
        runs.append((e, states, ubs))
    return runs


def assert_tick_matches(name, t, want, want_ubs, got, got_ub, sticky=False):
    """got (the device's state after tick t, 1004 bytes) against the oracle's; exact until the oracle first raises
    FLAME_QUEUE_RANGE, the flame queue's bytes excepted from then on.  sticky: got_ub is a batch env's ubflags, which gather
    every tick's flags since upload (pom_batch_status); else the tick's own"""
    so_far = int(np.bitwise_or.reduce(want_ubs[:t + 1]))
    held = bool(so_far & UB_FLAME_QUEUE_RANGE)
    w, g = np.frombuffer(want[t].tobytes(), np.uint8), np.frombuffer(bytes(got), np.uint8)
    w_ub = so_far if sticky else int(want_ubs[t])
    assert int(got_ub) == w_ub, f"{name} tick {t}: ubflags {int(got_ub):#x}, oracle {w_ub:#x}"
    if held:
        diff = np.nonzero(w[:QUEUE_BYTES.start] != g[:QUEUE_BYTES.start])[0]
    else:
        diff = np.nonzero(w != g)[0]
    assert diff.size == 0, f"{name} tick {t}: bytes {diff[:12].tolist()} differ from the oracle's (queue held: {held})"
    if held:  # what the record holds there: the reference's value where it fits, else the limit
        ws, gs = w[:1004].view(STATE_DTYPE)[0], g[:1004].view(STATE_DTYPE)[0]
        assert int(gs["flames_count"]) == min(int(ws["flames_count"]), 255)
        assert int(gs["flames_queue"]["timeLeft"].min()) >= -128


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_oracle_reproduces_the_reference_on_the_edge_corpus(oracle):
    """every tick the compiled reference played of every entry (tests/golden/gen_edge_cases.py): the oracle's state hash after
    it, and the full states at the checkpoints — the oracle, not only the device, is pinned on the >20-flame path"""
    g = np.load(GOLDEN)
    entries = corpus(oracle)
    assert [e.name for e in entries] == list(g["names"]), "the corpus changed: regenerate tests/golden/edge_cases.npz"
    ck = {(int(e), int(t)): g["ck_state"][k] for k, (e, t) in enumerate(zip(g["ck_entry"], g["ck_tick"]))}
    beyond_20 = beyond_255 = below_128 = 0
    for i, e in enumerate(entries):
        assert e.start.tobytes() == g["start"][i].tobytes(), e.name
        assert np.array_equal(e.moves, g["moves"][g["moff"][i]:g["moff"][i + 1]]), e.name
        s = e.start.copy()
        hashes = g["hashes"][g["hoff"][i]:g["hoff"][i + 1]]
        for t, h in enumerate(hashes):
            ub = oracle.step(s, e.moves[t])
            s["agents"]["pad"] = 0
            assert not ub & FATAL
            assert _hash(s.tobytes()) == int(h), f"{e.name}: the oracle leaves the reference at tick {t}"
            if (i, t + 1) in ck:
                assert s.tobytes() == ck[(i, t + 1)].tobytes(), f"{e.name}: checkpoint after tick {t}"
            beyond_20 += int(s["flames_count"][0]) > 20
            beyond_255 += int(s["flames_count"][0]) > 255
            below_128 += int(s["flames_queue"]["timeLeft"].min()) < -128
        if len(hashes) < len(e.moves):  # the reference was not given the next tick: the oracle predicts a crashing UB for it
            assert oracle.step(s.copy(), e.moves[len(hashes)]) & FATAL, e.name
    assert beyond_20 > 1000 and beyond_255 > 0 and below_128 > 0, (beyond_20, beyond_255, below_128)


def test_corpus_reaches_the_limits_it_is_about(edge_runs):
    seen = 0
    for e, states, ubs in edge_runs:
        assert (np.bitwise_or.reduce(ubs) & e.expect_ub) == e.expect_ub, f"{e.name}: flags {e.expect_ub:#x} expected"
        seen |= int(np.bitwise_or.reduce(ubs))
    assert seen & 0x27 == 0x27  # LOST_AGENT, NULL_BOMB, QUEUE_OVERFLOW, FLAME_QUEUE_RANGE
    by = {e.name: (states, ubs) for e, states, ubs in edge_runs}
    fin = lambda n: by[n][0][-1].view(STATE_DTYPE)[0]  # noqa: E731
    assert int(fin("bombcount_down_-108")["agents"]["bombCount"][2]) == -128
    assert int(fin("alive_-124")["aliveAgents"]) == -128
    assert max(int(s.view(STATE_DTYPE)[0]["agents"]["maxBombCount"][0]) for s in by["maxbombs_32646"][0]) == 32646 + 9
    assert max(int(s.view(STATE_DTYPE)[0]["agents"]["bombStrength"][3]) for s in by["strength_134"][0]) == 134 + 7


@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_device_tick_body_matches_oracle_on_the_edge_corpus(emul_bins, edge_runs, quad):  # noqa: F811
    """every tick of every entry, the record packed once and kept between ticks (what the device does): all 1004 bytes and
    ubflags against the oracle; the quad model's own checks hold"""
    run = emul_bins.pom_emul_run
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    run.restype = C.c_int
    for e, want, want_ubs in edge_runs:
        T = len(e.moves)
        got, ubs = np.zeros((T, 1004), dtype=np.uint8), np.zeros(T, dtype=np.uint32)
        mv = np.ascontiguousarray(e.moves, dtype=np.int32)
        assert run(e.start.ctypes.data, mv.ctypes.data, T, quad, got.ctypes.data, ubs.ctypes.data) == 0, e.name
        assert not (ubs & 0x40000000).any(), f"{e.name}: the quad model's checks failed"
        for t in range(T):
            assert_tick_matches(e.name, t, want, want_ubs, got[t].tobytes(), ubs[t])


# The two State -> record -> State paths (pomcpp_amd/csrc/pom_packed.h), as exports of the host build with pom_emul_step's signature:
# pom_pack_state / pom_unpack_state (upload and download of a batch), and the per-lane functions that pom_step's kernel runs.
PACKERS = {"pom_pack_state": "pom_emul_step", "pom_step": "pom_emul_step_one"}


def _pack_roundtrip(emul_bins, s, packer="pom_pack_state"):  # noqa: F811
    """pack -> unpack only (ENV mode on a finished env skips the tick): 0, or 0xFFFFFFFF if refused"""
    idle = np.zeros(4, dtype=np.int32)
    st = C.c_uint32(1)
    return getattr(emul_bins, PACKERS[packer])(s.ctypes.data, idle.ctypes.data, 1, 0, C.byref(st)) & 0xFFFFFFFF


# (field setter, value at the bound, value one step beyond)
def _agent(field, i=1):
    return lambda s, v: s["agents"][field].__setitem__((0, i), v)


def _flame(field, slot=3):
    return lambda s, v: s["flames_queue"][field].__setitem__((0, slot), v)


BOUNDS = [
    ("bombCount_min", _agent("bombCount"), -108, -109), ("bombCount_max", _agent("bombCount"), 107, 108),
    ("maxBombCount_min", _agent("maxBombCount"), -32768, -32769), ("maxBombCount_max", _agent("maxBombCount"), 32646, 32647),
    ("bombStrength_min", _agent("bombStrength"), 0, -1), ("bombStrength_max", _agent("bombStrength"), 134, 135),
    ("aliveAgents_min", lambda s, v: s["aliveAgents"].__setitem__(0, v), -124, -125),
    ("aliveAgents_max", lambda s, v: s["aliveAgents"].__setitem__(0, v), 127, 128),
    ("flames_count_max", lambda s, v: s["flames_count"].__setitem__(0, v), 255, 256),
    ("flames_count_min", lambda s, v: s["flames_count"].__setitem__(0, v), 0, -1),
    ("flames_index_max", lambda s, v: s["flames_index"].__setitem__(0, v), 19, 20),
    ("flame_timeLeft_min", _flame("timeLeft"), -128, -129), ("flame_timeLeft_max", _flame("timeLeft"), 127, 128),
    ("flame_strength_max", _flame("strength"), 255, 256), ("flame_x_max", _flame("x"), 10, 11),
    ("bombs_count_max", lambda s, v: s["bombs_count"].__setitem__(0, v), 20, 21),
    ("bombs_index_max", lambda s, v: s["bombs_index"].__setitem__(0, v), 19, 20),
]


# every bound through both packers (the ids of pom_pack_state's cases are the bounds' names alone)
BOUND_CASES = [pytest.param(packer, *b, id=b[0] if packer == "pom_pack_state" else f"{b[0]}-{packer}") for packer in PACKERS for b in BOUNDS]


@pytest.mark.parametrize("packer,name,poke,at,beyond", BOUND_CASES)
def test_packer_accepts_the_bound_and_refuses_one_beyond(emul_bins, packer, name, poke, at, beyond):  # noqa: F811
    import pomcpp_amd as pa
    s = pa.make_boards(1, seed=5)
    s["agents"]["pad"] = 0
    poke(s, at)
    before = s.copy()
    assert _pack_roundtrip(emul_bins, s, packer) == 0, f"{name}={at} refused"
    assert s.tobytes() == before.tobytes(), f"{name}={at} does not survive pack / unpack"
    poke(s, beyond)
    before = s.copy()
    assert _pack_roundtrip(emul_bins, s, packer) == 0xFFFFFFFF, f"{name}={beyond} accepted"
    assert s.tobytes() == before.tobytes()


# a bomb word (bboard.hpp:261-335: x:4 | y:4 | id:4 @8 | strength:4 @12 | time:4 @16) that fits its record dword like any other
# but cannot be a bomb of a game: off the board, or of an agent that does not exist
OFF_BOARD_BOMBS = [("x_11", 11 | (3 << 4) | (1 << 12) | (5 << 16)), ("y_11", 3 | (11 << 4) | (1 << 12) | (5 << 16)),
                   ("agent_4", 3 | (3 << 4) | (4 << 8) | (1 << 12) | (5 << 16))]


@pytest.mark.parametrize("name,word", OFF_BOARD_BOMBS, ids=[b[0] for b in OFF_BOARD_BOMBS])
def test_live_bomb_rule_is_what_pom_steps_packer_refuses_beyond_pom_pack_state(emul_bins, name, word):  # noqa: F811
    """The live-bomb rule (pom_pack_live_bomb_bad): a bomb in one of the bombs.count slots from bombs.index on must sit on the
    board and belong to a real agent.  It is the ONE place where pom_step's packer (and upload to a batch) is stricter than
    pom_pack_state, which keeps the bomb queue raw: the same word in a stale slot passes both, in a live slot only pom_pack_state."""
    import pomcpp_amd as pa
    s = pa.make_boards(1, seed=5)
    s["agents"]["pad"] = 0
    s["bombs_index"][0], s["bombs_count"][0] = 18, 3  # live: slots 18, 19, 0 (the queue wraps)
    s["bombs_queue"][0, [18, 19, 0]] = 3 | (3 << 4) | (1 << 12) | (5 << 16)
    for slot, live in ((1, False), (17, False), (18, True), (0, True)):
        t = s.copy()
        t["bombs_queue"][0, slot] = word
        for packer in PACKERS:
            before = t.copy()
            refused = live and packer == "pom_step"
            assert _pack_roundtrip(emul_bins, t, packer) == (0xFFFFFFFF if refused else 0), f"{packer}: {name} in slot {slot} (live: {live})"
            assert t.tobytes() == before.tobytes(), f"{packer}: {name} in slot {slot} altered"


# ---------------------------------------------------------------------------------------------------------------- GPU
def _batch(oracle, ticks):
    """every env of a ragged batch is a corpus entry (entry i at env 3i, and again at 3i + 1 and 3i + 2 shifted, so entries sit at
    lane 0, lane 15 and in the last, partial tile of 15); scripts padded with IDLE to `ticks`.  Returns start states, moves
    int32[ticks, n, 4], and the oracle's states uint8[ticks, n, 1004] and flags uint32[ticks, n] (Step only, RAW)."""
    entries = corpus(oracle)
    E = len(entries)
    order = [j for i in range(E) for j in (i, (i + 7) % E, (i + 13) % E)] + list(range(7))
    n = len(order)
    assert n % 16 == 15
    start = np.concatenate([entries[j].start for j in order])
    moves = np.zeros((ticks, n, 4), dtype=np.int32)
    for k, j in enumerate(order):
        m = entries[j].moves[:ticks]
        moves[:len(m), k] = m
    want, ubs = np.zeros((ticks, n, 1004), dtype=np.uint8), np.zeros((ticks, n), dtype=np.uint32)
    s = start.copy()
    for t in range(ticks):
        ubs[t] = oracle.step_batch(s, moves[t])
        s["agents"]["pad"] = 0
        want[t] = s.view(np.uint8).reshape(n, 1004)
    return [entries[j].name for j in order], start, moves, want, ubs


@pytest.fixture(scope="module")
def gpu_batch(oracle):
    return _batch(oracle, 160)


def _check_all(names, t, want, ubs, got_states, got_ubs):
    g = got_states.view(np.uint8).reshape(len(names), 1004)
    for k, name in enumerate(names):
        assert_tick_matches(f"{name} (env {k})", t, want[:, k], ubs[:, k], g[k].tobytes(), got_ubs[k], sticky=True)


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", [(16, 4), (16, 1), (32, 1), (64, 1)])
def test_edges_gpu_raw_step_every_tick(hip_lib, gpu_batch, epw, lpe):
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    names, start, moves, want, ubs = gpu_batch
    with BatchEnvironment(len(names), mode=MODE_RAW, envs_per_wave=epw, lanes_per_env=lpe) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        env.make_game(start)
        for t in range(len(moves)):
            env.step(moves[t])
            _check_all(names, t, want, ubs, env.get_state(), env.status()["ubflags"])


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", [(16, 4), (16, 1), (32, 1), (64, 1)])
def test_edges_gpu_env_step_every_tick(hip_lib, oracle, gpu_batch, epw, lpe):
    """ENV mode without auto-reset: Environment::Step's tick and bookkeeping; a finished game is not stepped again"""
    from pomcpp_amd.batch import MODE_ENV, BatchEnvironment
    names, start, moves, _, _ = gpu_batch
    n = len(names)
    ref = start.copy()
    status = [dict(done=0, winner=-1, draw=0) for _ in range(n)]
    ubs, wants = np.zeros((len(moves), n), dtype=np.uint32), []
    for t in range(len(moves)):
        for k in range(n):
            if not status[k]["done"]:
                ubs[t, k] = oracle.env_step(ref[k:k + 1], moves[t, k], status[k])
        ref["agents"]["pad"] = 0
        wants.append(ref.view(np.uint8).reshape(n, 1004).copy())
    want = np.stack(wants)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=False, envs_per_wave=epw, lanes_per_env=lpe) as env:
        env.make_game(start)
        for t in range(len(moves)):
            env.step(moves[t])
            st = env.status()
            _check_all(names, t, want, ubs, env.get_state(), st["ubflags"])
        assert [bool(d) for d in st["done"]] == [bool(s["done"]) for s in status]
        assert [int(w) for w in st["winner"]] == [s["winner"] for s in status]


@pytest.mark.gpu
def test_edges_gpu_tape_observe_and_range(hip_lib, gpu_batch):
    """the chained tape (step_device_many, in pieces of 1..37 ticks), step + observation in one launch, and the closed-loop
    range call: the same states as the oracle's at every point they can be looked at"""
    import torch
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    names, start, moves, want, ubs = gpu_batch
    n, K = len(names), len(moves)
    dev_moves = torch.from_numpy(moves).to("cuda:0")
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(start)
        t = 0
        for piece in (1, 2, 37, 5, 20, 3, 32, 60):
            piece = min(piece, K - t)
            if piece <= 0:
                break
            env.step_device_many(dev_moves[t:t + piece].contiguous())
            env.sync()
            t += piece
            _check_all(names, t - 1, want, ubs, env.get_state(), env.status()["ubflags"])
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(start)
        for t in range(40):
            env.step_device_observe(dev_moves[t].contiguous())
            env.sync()
            _check_all(names, t, want, ubs, env.get_state(), env.status()["ubflags"])
    whole = n - n % 16
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(start[:])
        env.sync()
        for t in range(40):
            env.step_device_range(0, whole, dev_moves[t].contiguous())
            env.step_device_range(whole, n - whole, dev_moves[t].contiguous())
            env.sync()
            _check_all(names, t, want, ubs, env.get_state(), env.status()["ubflags"])


@pytest.mark.gpu
def test_edges_gpu_one_state_calls(hip_lib, oracle):
    """pom_step / pom_env_step (a kernel of their own): every entry, every tick, from the state the previous call left (the
    record is re-packed each call, so an entry stops at the first state upload refuses)"""
    from pomcpp_amd.batch import PomError, env_step_one, step_one
    for e in corpus(oracle):
        a, g = e.start.copy(), e.start.copy()
        st = dict(done=0, winner=-1, draw=0)
        for t, mv in enumerate(e.moves[:60]):
            ub = oracle.step(a, mv)
            a["agents"]["pad"] = 0
            try:
                step_one(g, mv)
            except PomError as err:  # the previous tick left a state beyond upload's bounds
                assert err.code == 3 and t > 0, (e.name, err.code)  # POM_E_UNREPRESENTABLE
                break
            if ub & UB_FLAME_QUEUE_RANGE:
                break
            assert g.tobytes() == a.tobytes(), f"{e.name} tick {t}: pom_step differs from the oracle"
        b, h = e.start.copy(), e.start.copy()
        for t, mv in enumerate(e.moves[:60]):
            ub = oracle.env_step(b, mv, st)
            b["agents"]["pad"] = 0
            try:
                r = env_step_one(h, mv)
            except PomError as err:
                assert err.code == 3 and t > 0, (e.name, err.code)
                break
            if ub & UB_FLAME_QUEUE_RANGE:
                break
            assert h.tobytes() == b.tobytes() and r["ubflags"] == ub and r["done"] == st["done"], f"{e.name} tick {t}: pom_env_step"
            if st["done"]:
                break


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "float16", "float32", "codes"])
def test_edges_gpu_observation_of_the_corpus(hip_lib, gpu_batch, dtype):
    """the observation of the corpus states (stuck queues: every timeLeft negative; plane 15 clamps) against
    oracle/pom_observe_oracle.py, at the start, after 24 ticks and after the last"""
    import importlib.util
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    ob = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ob)
    names, start, moves, _, _ = gpu_batch
    with BatchEnvironment(len(names), mode=MODE_RAW) as env:
        env.make_game(start)
        for t in range(len(moves) + 1):
            if t in (0, 24, len(moves)):
                states = env.get_state()
                if dtype == "codes":
                    got = env.observe(dtype="codes")[0].cpu().numpy()
                    assert np.array_equal(got, ob.observe_codes(states)), t
                else:
                    for per_agent in (False, True):
                        got, attrs, _ = env.observe(per_agent=per_agent, dtype=dtype)
                        want, want_attrs, _ = ob.observe(states, per_agent=per_agent, dtype=getattr(np, dtype))
                        assert np.array_equal(got.cpu().numpy(), want), (t, per_agent)
                        assert np.array_equal(attrs.cpu().numpy(), want_attrs)
            if t < len(moves):
                env.step(moves[t])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["at_start", "at_end"])
def test_edges_gpu_env_auto_reset_every_tick(hip_lib, oracle, gpu_batch, mode):
    """ENV mode with auto-reset and max_steps 23: entries finish by their scripts or are cut in the middle of them, restart from
    their start states and play on (the moves of tick t are row t of the padded scripts, whichever episode it falls in).  The
    model: oracle.env_step, and the start state on a restart.  Every tick: the states, ubflags (they gather the flags of the
    current episode: a restart clears them, pom_batch.h), done / winner, with RESET_AT_END the finished marks, last results and
    terminal states; at the end the step, episode and reset counters."""
    from pomcpp_amd.batch import (CNT_EPISODES, CNT_RESETS, CNT_STEPS, MODE_ENV, RESET_AT_END, RESET_AT_START,
                                  BatchEnvironment)
    names, start, moves, _, _ = gpu_batch
    n, cap, T = len(names), 23, 100
    at_end = mode == "at_end"
    ref = start.copy()
    status = [dict(done=0, winner=-1, draw=0) for _ in range(n)]
    acc = np.zeros(n, dtype=np.uint32)  # the current episode's flags
    term, term_acc = np.zeros(n, dtype=STATE_DTYPE), np.zeros(n, dtype=np.uint32)
    last = dict(winner=np.full(n, -1), draw=np.zeros(n, int), length=np.zeros(n, int), alive=np.zeros(n, int))
    finished_total = restarts = 0
    fin_prev = np.zeros(n, dtype=bool)

    def compare(what, t, k, got, want, ub_acc):
        g, w = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
        end = QUEUE_BYTES.start if ub_acc & UB_FLAME_QUEUE_RANGE else 1004
        diff = np.nonzero(g[:end] != w[:end])[0]
        assert diff.size == 0, f"{names[k]} (env {k}) tick {t}: {what} bytes {diff[:12].tolist()} differ"

    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END if at_end else RESET_AT_START, max_steps=cap) as env:
        env.make_game(start)
        for t in range(T):
            mv = moves[t % len(moves)]
            fin = np.zeros(n, dtype=bool)
            for k in range(n):
                if not at_end and fin_prev[k]:  # RESET_AT_START: the tick first puts the env back on its start state
                    ref[k] = start[k]
                    status[k] = dict(done=0, winner=-1, draw=0)
                    acc[k] = 0
                    restarts += 1
                acc[k] |= oracle.env_step(ref[k:k + 1], mv[k], status[k])
                fin[k] = bool(status[k]["done"]) or int(ref["timeStep"][k]) >= cap
                if fin[k] and at_end:
                    last["winner"][k], last["draw"][k] = status[k]["winner"], status[k]["draw"]
                    last["length"][k], last["alive"][k] = ref["timeStep"][k], ref["aliveAgents"][k]
                    ref["agents"]["pad"][k] = 0
                    term[k], term_acc[k] = ref[k], acc[k]
                    ref[k] = start[k]
                    status[k] = dict(done=0, winner=-1, draw=0)
                    acc[k] = 0
                    restarts += 1
            ref["agents"]["pad"] = 0
            finished_total += int(fin.sum())
            fin_prev = fin
            env.step(mv)
            got, st = env.get_state(), env.status()
            for k in range(n):
                compare("state", t, k, got[k], ref[k], acc[k])
            assert st["ubflags"].tolist() == acc.tolist(), f"tick {t}: ubflags"
            if at_end:
                r = env.last_results()
                assert r["finished"].astype(bool).tolist() == fin.tolist(), f"tick {t}: finished"
                for key in ("winner", "draw", "length", "alive"):
                    assert r[key].tolist() == last[key].tolist(), (t, key)
                assert not st["done"].any()
                gt = env.get_terminal_state()
                for k in np.nonzero(fin)[0]:
                    compare("terminal state", t, k, gt[k], term[k], term_acc[k])
            else:
                assert st["done"].astype(bool).tolist() == fin.tolist(), f"tick {t}: done"
                assert st["winner"].tolist() == [s["winner"] for s in status], f"tick {t}: winner"
        cnt = env.counters()
    assert finished_total > n and restarts > n
    assert cnt[CNT_STEPS] == n * T
    assert cnt[CNT_EPISODES] == finished_total and cnt[CNT_RESETS] == restarts
