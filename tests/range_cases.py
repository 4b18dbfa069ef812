"""TEST INFRASTRUCTURE — the cases of tests/test_range_modes.py (GPU) and tests/test_range_model_host.py (CPU): handles of 200 envs at
env_offset 1000 (twelve whole tiles and a short one of 8) cut into the ranges (0, 16) — one workgroup —, (16, 144) — nine tiles: more
than one per XCD and a remainder modulo 8 — and (160, 40) — two tiles and the short one, up to the batch's end; one case of 40 envs.
A case names the handle's options and its boards; its schedule — about 30 rounds, each calling a seeded subset of the ranges in a
seeded order, some of them twice in a row, every call with its own random moves 0..5 — is a function of the case alone, so that the
CPU test can assert from the model what the schedule contains before the GPU test relies on it."""
import numpy as np

from tests.range_model import RangeModel, RESET_OFF, RESET_AT_START, RESET_AT_END

N, ENV_OFFSET, BSEED, ROUNDS = 200, 1000, 5, 30
RANGES = ((0, 16), (16, 144), (160, 40))
SMALL_N, SMALL_RANGES = 40, ((0, 16), (16, 24))
MODES = ((RESET_OFF, False), (RESET_AT_START, False), (RESET_AT_START, True), (RESET_AT_END, False), (RESET_AT_END, True))
UB_SEED = 9    # stress boards of this seed raise UB flags within the ticks played (asserted by the CPU test)


def _case(reset, fresh, cap, boards, n=N, ranges=RANGES, seed=0):
    name = f"{('off', 'at_start', 'at_end')[reset]}-{'fresh' if fresh else 'snapshot'}-cap{cap}-{boards}-n{n}"
    return dict(name=name, reset=reset, fresh=fresh, cap=cap, boards=boards, n=n, ranges=ranges, seed=seed)


# every mode at max_steps 3 (new boards; generated ones where the restarts generate) and at 800 (burned-in boards: natural ends)
CASES = [_case(reset, fresh, 3, "generated" if fresh else "new") for reset, fresh in MODES]
CASES += [_case(reset, fresh, 800, "burned") for reset, fresh in MODES]
CASES += [_case(RESET_AT_END, True, 800, "stress"), _case(RESET_AT_END, True, 3, "generated", SMALL_N, SMALL_RANGES)]
CASE_IDS = [c["name"] for c in CASES]

_boards = {}


def boards_of(oracle, case):
    """the case's start boards, computed once and shared (never changed)"""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import DIST_STRESS
    from tests.test_visit_path import burned_in
    key = (case["boards"], case["n"])
    if key not in _boards:
        n = case["n"]
        if case["boards"] == "new":
            b = pa.make_boards(n, seed=41 + n)
        elif case["boards"] == "generated":
            b = oracle.boardgen(BSEED, np.arange(n) + ENV_OFFSET, np.zeros(n))
        elif case["boards"] == "burned":
            b = burned_in(oracle, n, 41 + n)
        elif case["boards"] == "stress0":
            b = pa.make_boards(n, seed=8, kind="stress")
        else:
            b = burned_in(oracle, n, UB_SEED, kind="stress", dist=DIST_STRESS, ticks=25)
        b = b.copy()
        b["agents"]["pad"] = 0
        _boards[key] = b
    return _boards[key]


def options_of(case):
    """BatchEnvironment's keyword arguments"""
    from pomcpp_amd.batch import MODE_ENV
    return dict(mode=MODE_ENV, auto_reset=case["reset"], max_steps=case["cap"], env_offset=ENV_OFFSET, fresh_boards=case["fresh"],
                board_seed=BSEED)


def model_of(oracle, case, cls=RangeModel):
    return cls(oracle, boards_of(oracle, case), max_steps=case["cap"], auto_reset=case["reset"], fresh_boards=case["fresh"],
               board_seed=BSEED, env_offset=ENV_OFFSET)


def schedule(case, rounds=ROUNDS):
    """[(index of the range, moves int32 [n, 4])]: the calls of the case, in order"""
    rng = np.random.default_rng([case["seed"], case["cap"], case["reset"], int(case["fresh"]), case["n"]])
    k, calls = len(case["ranges"]), []
    for _ in range(rounds):
        chosen = [int(i) for i in rng.permutation(k) if rng.random() < (0.9, 0.55, 0.75)[i]]   # the ranges drift apart
        for i in chosen or [int(rng.integers(k))]:
            for _ in range(2 if rng.random() < 0.3 else 1):      # some of them twice in a row
                calls.append((i, rng.integers(0, 6, size=(case["n"], 4), dtype=np.int32)))
    return calls


def play(oracle, case, cls=RangeModel):
    """the model after the case's whole schedule"""
    m = model_of(oracle, case, cls)
    for i, moves in schedule(case):
        m.tick(*case["ranges"][i], moves)
    return m


# ---- two streams out of lockstep: per round stream A carries three ticks of range 0 and two of range 2, stream B one tick of range 1
STREAM_A, STREAM_B, STREAM_ROUNDS = (0, 2, 0, 2, 0), (1,), 8
STREAM_CASES = [_case(RESET_AT_END, True, 4, "generated", seed=1), _case(RESET_AT_START, False, 4, "new", seed=1)]


def stream_schedule(case, rounds=STREAM_ROUNDS):
    """[round][stream A's calls, stream B's calls], a call = (index of the range, moves); the ranges do not overlap, so the model may
    play a round's calls in any order that keeps each stream's"""
    rng = np.random.default_rng([7, case["reset"], int(case["fresh"])])
    moves = lambda: rng.integers(0, 6, size=(case["n"], 4), dtype=np.int32)  # noqa: E731
    return [([(i, moves()) for i in STREAM_A], [(i, moves()) for i in STREAM_B]) for _ in range(rounds)]


# ---- the fused observation: reset at the end of the tick and a low bound, so that restarted envs are observed; stress boards (bombs and
# flames from the first tick on), not yet played
OBS_CASE, OBS_ROUNDS = _case(RESET_AT_END, False, 9, "stress0", seed=2), 16

# ---- next to chained calls: CHAIN_TICKS ticks of pom_batch_step_random from tick CHAIN_TICK0, a tick of every range, CHAIN_TICKS more
CHAIN_SEED, CHAIN_TICK0, CHAIN_TICKS, CHAIN_RANGES = 23, 7, 20, (1, 0, 2)


def chain_case(reset):
    return _case(reset, False, 80, "burned")


def chain_range_ticks(case):
    rng = np.random.default_rng([11, case["reset"]])
    return [(i, rng.integers(0, 6, size=(case["n"], 4), dtype=np.int32)) for i in CHAIN_RANGES]
