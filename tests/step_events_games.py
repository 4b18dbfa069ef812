"""TEST INFRASTRUCTURE — the games of tests/test_step_events_host.py (CPU) and tests/test_gpu_step_events.py (GPU): handles of N = 48 envs
(three whole tiles) that play TICKS ticks of pom_batch_step_events in each reset mode, agent 0 on seeded random moves and SimpleAgent in
the other three seats (one game with agents 1 and 3 on the caller's moves too).  The boards: generated ones (wood with hidden items:
gains, burnt wood) in the first 24 envs, the stress boards of tests/range_cases.py (bombs and flames from the first tick: chains, deaths,
UB flags) in the others.  Most calls cover the whole batch, every fifth one the middle tile alone, so that a record's rows outside a
range are seen to stay.  A function of the game alone, played once per model class and shared: the CPU test asserts what the record
holds — every bit of the header's table — before the GPU test compares the kernel with it."""
import numpy as np

from tests import range_cases as RC
from tests.range_model import RESET_AT_END, RESET_AT_START, RESET_OFF
from tests.step_events_oracle import EventsModel

N, TICKS, SEED, TICK0 = 48, 120, 777, 4_294_967_296 - 120   # (the calls' ticks run up to the top of the 32 bits the spec takes)


def _game(reset, fresh, cap, mask):
    return dict(name=f"{('off', 'at_start', 'at_end')[reset]}-{'fresh' if fresh else 'snapshot'}-cap{cap}-mask{mask:x}", reset=reset, fresh=fresh,
                cap=cap, mask=mask)


GAMES = [_game(RESET_OFF, False, 70, 0b1110), _game(RESET_AT_START, True, 45, 0b1110), _game(RESET_AT_END, False, 45, 0b1010),
         _game(RESET_AT_END, True, 60, 0b1110), _game(RESET_AT_START, False, 800, 0b0010)]   # (the last: three random movers raise UB flags)
GAME_IDS = [g["name"] for g in GAMES]
_cache = {}


def boards_of(oracle):
    if "boards" not in _cache:
        b = np.concatenate([oracle.boardgen(RC.BSEED, np.arange(24) + RC.ENV_OFFSET, np.zeros(24)),
                            RC.boards_of(oracle, dict(boards="stress", n=24))])
        b["agents"]["pad"] = 0
        _cache["boards"] = b
    return _cache["boards"]


def options_of(game):
    """BatchEnvironment's keyword arguments"""
    from pomcpp_amd.batch import MODE_ENV
    return dict(mode=MODE_ENV, auto_reset=game["reset"], max_steps=game["cap"], env_offset=RC.ENV_OFFSET, fresh_boards=game["fresh"],
                board_seed=RC.BSEED)


def calls_of(game, ticks=TICKS):
    """[(first, count, moves int32 [N, 4], tick)]"""
    rng = np.random.default_rng([31, game["reset"], int(game["fresh"]), game["cap"], game["mask"]])
    return [((16, 16) if t % 5 == 4 else (0, N)) + (rng.integers(0, 6, size=(N, 4), dtype=np.int32), TICK0 + t) for t in range(ticks)]


def play(oracle, game, cls=EventsModel, ticks=TICKS):
    """dict(model, ticks=[dict(range, events, outcome, wood)]): the game played by a model of `cls`, once, and shared (never changed)"""
    key = (game["name"], cls, ticks)
    if key not in _cache:
        m = cls(oracle, boards_of(oracle), max_steps=game["cap"], auto_reset=game["reset"], fresh_boards=game["fresh"], board_seed=RC.BSEED,
                env_offset=RC.ENV_OFFSET)
        out = []
        for first, count, moves, tick in calls_of(game, ticks):
            if hasattr(m, "tick_events"):
                m.tick_events(first, count, moves, game["mask"], SEED, tick)
                out.append(dict(m.record(), range=(first, count)))
            else:
                m.tick_mixed(first, count, moves, game["mask"], SEED, tick)
                out.append(dict(range=(first, count)))
        _cache[key] = dict(model=m, ticks=out)
    return _cache[key]
