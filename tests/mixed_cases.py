"""TEST INFRASTRUCTURE — the cases of tests/test_step_mixed.py (GPU) and tests/test_mixed_model_host.py (CPU): the shapes of
tests/range_cases.py — 200 envs at env_offset 1000 cut into (0, 16), (16, 144) and (160, 40), and the case of 40 envs — under
pom_batch_step_mixed.  A case names the handle's options, its boards and the mask; every handle first plays PRE ticks of
pom_batch_step_simple from handle tick PRE_TICK0, so that ALL agents have memory when the first mixed call comes; then the schedule:
rounds that call a seeded subset of the ranges in a seeded order, some twice in a row, every call with its own random moves 0..5 and
the range's OWN tick counter (range i starts at RANGE_TICK0[i] and counts its own calls: the ranges run out of lockstep).  A function
of the case alone, so that the CPU test can assert what a schedule contains before the GPU test relies on it.

Boards: "burned" ones (60 ticks of random play behind them: dead agents, bombs, games of every age) under max_steps 40 — every third
game is over after its first tick, the others end one by one —, generated ones where the restarts generate, the stress boards that
raise UB flags, and "crowded" ones: the four agents on cells of a 3 x 3 corner of an empty board, one or two of them dead — where a
dead agent stands in the way and its Move[4] entry decides who may walk (step_utility.cpp:154-172), so that a dead agent of the mask
that does not idle shows at once; max_steps 4 puts the envs back there every few ticks."""
import numpy as np

from tests import range_cases as RC
from tests.mixed_model import MixedModel
from tests.range_model import RESET_AT_START, RESET_AT_END

SEED, PRE, PRE_TICK0, ROUNDS = 12345, 5, 3, 12
RANGE_TICK0 = (1000, 50, 4_000_000_000)   # per range; the last one counts up to the top of the 32 bits the spec takes
MASKS = (0b1110, 0b0101, 0xF, 0)


def _case(reset, fresh, mask, cap=40, boards="burned", n=RC.N, ranges=RC.RANGES):
    c = RC._case(reset, fresh, cap, boards, n, ranges, seed=3)
    c.update(mask=mask, name=f"{c['name']}-mask{mask:x}")
    return c


CASES = [_case(reset, fresh, mask) for reset, fresh in RC.MODES for mask in MASKS]
CASES += [_case(RESET_AT_START, False, 0b0010, 800, "stress"), _case(RESET_AT_END, True, 0b1110, 6, "generated", RC.SMALL_N, RC.SMALL_RANGES)]
CASES += [_case(reset, False, mask, 4, "crowded", RC.SMALL_N, RC.SMALL_RANGES) for reset, mask in ((RESET_AT_START, 0b1110), (RESET_AT_END, 0b0101))]
CASE_IDS = [c["name"] for c in CASES]
_crowded = {}


def boards_of(oracle, case):
    """the case's start boards, computed once and shared (never changed): tests/range_cases.py's, or the crowded ones"""
    if case["boards"] != "crowded":
        return RC.boards_of(oracle, case)
    if case["n"] not in _crowded:
        from pomcpp_amd import state as S
        rng, b = np.random.default_rng(17), S.new_states(case["n"])
        for e in range(case["n"]):
            for a, cell in enumerate(rng.permutation(9)[:4]):
                S.put_agent(b[e], int(cell) % 3, int(cell) // 3, a)
            dead = {int(rng.integers(4)), int(rng.integers(4))}   # one or two dead agents: of every mask's in most envs
            S.kill(b[e], *dead)
            for a in dead:   # as after a death in the flames: gone from the board, the stale position stays with the agent
                S.put_item(b[e], int(b["agents"]["x"][e, a]), int(b["agents"]["y"][e, a]), 0)
        b["agents"]["pad"] = 0
        _crowded[case["n"]] = b
    return _crowded[case["n"]]


def model_of(oracle, case, cls=MixedModel, pre=True):
    """the model of the case's handle after its PRE ticks of step_simple"""
    m = cls(oracle, boards_of(oracle, case), max_steps=case["cap"], auto_reset=case["reset"], fresh_boards=case["fresh"],
            board_seed=RC.BSEED, env_offset=RC.ENV_OFFSET)
    if pre:
        m.handle_tick = PRE_TICK0
        m.simple_ticks(SEED, PRE)
    return m


def schedule(case, rounds=ROUNDS):
    """[(index of the range, moves int32 [n, 4], the call's tick)]: the calls of the case, in order"""
    rng = np.random.default_rng([case["seed"], case["cap"], case["reset"], int(case["fresh"]), case["n"], case["mask"]])
    k, calls, ticks = len(case["ranges"]), [], list(RANGE_TICK0)
    for _ in range(rounds):
        chosen = [int(i) for i in rng.permutation(k) if rng.random() < (0.9, 0.6, 0.75)[i]]   # the ranges drift apart
        for i in chosen or [int(rng.integers(k))]:
            for _ in range(2 if rng.random() < 0.3 else 1):      # some of them twice in a row
                calls.append((i, rng.integers(0, 6, size=(case["n"], 4), dtype=np.int32), ticks[i]))
                ticks[i] += 1
    return calls


def play(oracle, case, cls=MixedModel):
    """the model after the case's whole schedule"""
    m = model_of(oracle, case, cls)
    m.before = dict(memory=m.mems.copy(), calls=len(m.calls))   # what stood when the first mixed call came
    for i, moves, tick in schedule(case):
        m.tick_mixed(*case["ranges"][i], moves, case["mask"], SEED, tick)
    return m


# ---- two streams out of lockstep (tests/range_cases.py's shape): per round stream A carries three ticks of range 0 and two of range 2,
# stream B one tick of range 1
STREAM_CASES = [_case(RESET_AT_END, True, 0b1110, 8, "generated"), _case(RESET_AT_START, False, 0b0101)]
STREAM_ROUNDS = 6


def stream_schedule(case, rounds=STREAM_ROUNDS):
    """[round][stream A's calls, stream B's calls], a call = (index of the range, moves, tick)"""
    rng = np.random.default_rng([7, case["reset"], int(case["fresh"]), case["mask"]])
    ticks = list(RANGE_TICK0)

    def call(i):
        ticks[i] += 1
        return i, rng.integers(0, 6, size=(case["n"], 4), dtype=np.int32), ticks[i] - 1
    return [([call(i) for i in RC.STREAM_A], [call(i) for i in RC.STREAM_B]) for _ in range(rounds)]
