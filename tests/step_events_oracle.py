"""TEST INFRASTRUCTURE — the checker of pom_batch_step_events (include/pom_batch.h PomStepEventsSpec): the header's rule as a literal
function of (S0, m, S1, status) on boundary States, and EventsModel, tests/mixed_model.py's host model of the handle with the three
arrays of every call on record.  Plain numpy on the States the CPU checker (Oracle.env_step) leaves; nothing of the kernel is restated:
no tile, no lane, no packed word.

The hooks (_s1_of, _event_moves, _laid) are there for the deliberately wrong variants of tests/test_step_events_host.py."""
import numpy as np

from tests.mixed_model import MixedModel
from tests.range_model import RESET_AT_START

# the header's POM_EV_* and POM_RO_*, restated as numbers: the tests do not take them from the package under test
MOVE, PLAYED, ALIVE, DIED, MOVED, LAID, GAIN_BOMB, GAIN_RANGE, GAIN_KICK, RESTARTED = 0x7, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800
EXPLODED_SHIFT, END, WON, DRAW, TIMEOUT, UB = 12, 0x10000, 0x20000, 0x40000, 0x80000, 0x100000
RO_DONE, RO_DRAW, RO_TIMEOUT, RO_UB, RO_WINNER_SHIFT, RO_LENGTH_SHIFT = 0x10, 0x20, 0x40, 0x80, 8, 16
BOMB = 5
BITS = dict(played=PLAYED, alive=ALIVE, died=DIED, moved=MOVED, laid=LAID, gain_bomb=GAIN_BOMB, gain_range=GAIN_RANGE, gain_kick=GAIN_KICK,
            restarted=RESTARTED, end=END, won=WON, draw=DRAW, timeout=TIMEOUT, ub=UB)
SENTINEL_EVENTS, SENTINEL_OUTCOME, SENTINEL_WOOD = 0xDEADBEEF, 0xFEEDFACE, 0xA5   # what the rows no call has written hold


def clamp(m):
    """a move as the tick's clamp leaves it"""
    return int(m) if 0 <= int(m) <= 5 else 6


def status_of(done=0, winner=-1, draw=0, timeout=0, ub=0, end=False, restarted=False):
    """the status a tick left, as the checker takes it: Environment's done / winner / draw, the time-out, this tick's UB flags, whether
    THIS tick finished the episode (POM_MODE_ENV only), whether the env restarted at the start of the call"""
    return dict(done=int(done), winner=int(winner), draw=int(draw), timeout=int(timeout), ub=int(ub), end=bool(end), restarted=bool(restarted))


def is_wood(board):
    return (np.asarray(board) >> 8) == 2


def event_words(s0, m, s1, status, laid=None):
    """events[e][0..3] of an env that played a tick: the table of the header, row by row"""
    out = []
    for a in range(4):
        a0, a1 = s0["agents"][a], s1["agents"][a]
        mv = clamp(m[a])
        alive0, alive1 = not a0["dead"], not a1["dead"]
        lay = alive0 and mv == BOMB and int(a0["bombCount"]) < int(a0["maxBombCount"])
        if laid is not None:
            lay = laid(a0, mv)
        w = mv | PLAYED
        w |= ALIVE if alive1 else 0
        w |= DIED if alive0 and not alive1 else 0
        w |= MOVED if alive0 and (int(a0["x"]), int(a0["y"])) != (int(a1["x"]), int(a1["y"])) else 0
        w |= LAID if lay else 0
        w |= GAIN_BOMB if int(a1["maxBombCount"]) > int(a0["maxBombCount"]) else 0
        w |= GAIN_RANGE if int(a1["bombStrength"]) > int(a0["bombStrength"]) else 0
        w |= GAIN_KICK if a1["canKick"] and not a0["canKick"] else 0
        w |= RESTARTED if status["restarted"] else 0
        w |= min(max(int(a0["bombCount"]) + int(lay) - int(a1["bombCount"]), 0), 15) << EXPLODED_SHIFT
        if status["end"]:
            w |= END
            w |= WON if status["winner"] == a else 0
            w |= DRAW if status["draw"] else 0
            w |= TIMEOUT if status["timeout"] else 0
        w |= UB if status["ub"] else 0
        out.append(w)
    return out


def idle_words(s):
    """events[e][0..3] of an env of the range that is not ticked"""
    return [0 if s["agents"][a]["dead"] else ALIVE for a in range(4)]


def outcome_word(s1, status):
    """outcome[e]: the POM_RO_* word of S1"""
    w = sum(1 << a for a in range(4) if not s1["agents"][a]["dead"])
    w |= RO_DONE if status["done"] else 0
    w |= RO_DRAW if status["draw"] else 0
    w |= RO_TIMEOUT if status["timeout"] else 0
    w |= RO_UB if status["ub"] else 0
    w |= (status["winner"] + 1) << RO_WINNER_SHIFT
    return w | min(int(s1["timeStep"]), 65535) << RO_LENGTH_SHIFT


def wood_burnt(s0, s1):
    """wood[e]: cells that are wood in S0 and not in S1"""
    return min(int((is_wood(s0["board"]) & ~is_wood(s1["board"])).sum()), 255)


def decode(word):
    """an event word's fields by name (for messages and for counting which bits a record holds)"""
    out = {k: bool(word & b) for k, b in BITS.items()}
    out.update(move=word & MOVE, exploded=word >> EXPLODED_SHIFT & 0xF)
    return out


class _Tap:
    """the CPU checker, with every Environment::Step it plays for the model put on the model's record"""

    def __init__(self, oracle, model):
        self._oracle, self._model = oracle, model

    def __getattr__(self, name):
        return getattr(self._oracle, name)

    def env_step(self, state, moves, status):
        ub = self._oracle.env_step(state, moves, status)
        self._model._played(state[0].copy(), dict(status), ub)
        return ub


class EventsModel(MixedModel):
    """MixedModel under pom_batch_step_events: tick_events() is tick_mixed() that also fills `events` uint32 [n, 4], `outcome` uint32 [n]
    and `wood` uint8 [n] for the rows of the range — the handle's state is tick_mixed()'s, untouched by the bookkeeping here"""

    def __init__(self, oracle, start, **options):
        super().__init__(oracle, start, **options)
        self.oracle = _Tap(oracle, self)
        self.events = np.full((self.n, 4), SENTINEL_EVENTS, np.uint32)
        self.outcome = np.full(self.n, SENTINEL_OUTCOME, np.uint32)
        self.wood = np.full(self.n, SENTINEL_WOOD, np.uint8)
        self._ticks, self._open = None, None

    # ---- where a kernel could go wrong (the wrong variants override these) ----------------------------------------------------
    def _s1_of(self, e, s1):
        """S1: what the tick left, BEFORE a restart at the end"""
        return s1

    def _event_moves(self, e, handed, callers, mask):
        """m: the moves handed to the tick"""
        return handed

    _laid = None   # (a0, move) -> bool in place of the header's LAID

    # ---- the record ----------------------------------------------------------------------------------------------------------------
    def _moves_of(self, e, first, moves, mask, seed, tick):
        # called once per env that plays, on S0 (behind the restart at the start), and returns m
        s0 = self.states[e].copy()
        handed = super()._moves_of(e, first, moves, mask, seed, tick)
        self._open = dict(e=e, s0=s0, m=np.array(handed), callers=None if moves is None else np.array(moves[e]), mask=mask)
        return handed

    def _played(self, s1, st, ub):
        if self._ticks is not None:   # (None: a tick of tick_mixed() / simple_ticks(), which keeps no record)
            self._ticks.append(dict(self._open, s1=s1, st=st, ub=ub))

    def tick_events(self, first, count, moves, mask, seed, tick):
        self._ticks = []
        was_done = self.done.copy()
        log = self.tick_mixed(first, count, moves, mask, seed, tick)
        ticked = set()
        for rec in self._ticks:
            e, s1 = rec["e"], rec["s1"]
            ticked.add(e)
            timeout = self.max_steps > 0 and int(s1["timeStep"]) >= self.max_steps
            done = bool(rec["st"]["done"] or timeout)
            status = status_of(done, rec["st"]["winner"], rec["st"]["draw"], timeout, rec["ub"], end=done,
                               restarted=bool(was_done[e]) and self.auto_reset == RESET_AT_START)
            s1 = self._s1_of(e, s1)
            self.events[e] = event_words(rec["s0"], self._event_moves(e, rec["m"], rec["callers"], rec["mask"]), s1, status, self._laid)
            self.outcome[e] = outcome_word(s1, status)
            self.wood[e] = wood_burnt(rec["s0"], s1)
        for e in range(first, first + count):
            if e not in ticked:   # finished, and no restart at the start: the state as it stands
                self.events[e] = idle_words(self.states[e])
                self.outcome[e] = outcome_word(self.states[e], status_of(self.done[e], self.winner[e], self.draw[e], self.timeout[e]))
                self.wood[e] = 0
        self._ticks = None
        return log

    def record(self):
        return dict(events=self.events.copy(), outcome=self.outcome.copy(), wood=self.wood.copy())
