"""TEST INFRASTRUCTURE — hand-made transitions for pom_batch_step_events (include/pom_batch.h PomStepEventsSpec), at least one per clause
of its rule, with the expected words written down as numbers worked out from the header's table and the reference's Step by hand — not
taken from any code.  tests/test_step_events_host.py runs them through the checker of tests/step_events_oracle.py on the CPU checker's
transitions (and on the compiled reference's where it was built); tests/test_gpu_step_events.py runs them through the kernel.

A case is (name, mode, build, ticks): build(oracle) returns the State the env starts from (agents 0..3 in the corners (0,0), (10,0),
(10,10), (0,10) unless said otherwise); ticks is a list of (moves, events[4], outcome, wood) — the calls the env gets, in order, on a
handle of POM_MODE_ENV ("env": max_steps CAP, no auto-reset, so a finished env is not ticked again) or POM_MODE_RAW ("raw").

The bits, for reading the numbers: move 0..2 (IDLE 0, UP 1, DOWN 2, LEFT 3, RIGHT 4, BOMB 5), PLAYED 0x8, ALIVE 0x10, DIED 0x20, MOVED 0x40,
LAID 0x80, GAIN_BOMB 0x100, GAIN_RANGE 0x200, GAIN_KICK 0x400, RESTARTED 0x800, EXPLODED 0xF000, END 0x10000, WON 0x20000, DRAW 0x40000,
TIMEOUT 0x80000, UB 0x100000.  Outcome: alive mask 0xF, DONE 0x10, DRAW 0x20, TIMEOUT 0x40, UB 0x80, winner + 1 at bit 8, timeStep at bit 16."""
import pomcpp_amd.state as S
from pomcpp_amd.state import Item

CAP = 800
IDLE, UP, DOWN, LEFT, RIGHT, BOMB = range(6)
IDLE4 = (IDLE,) * 4


def _base(*dead):
    s = S.new_states(1)
    S.put_agents_in_corners(s[0])
    for a in dead:   # as after a death in the flames: gone from the board, the position stays with the agent
        S.kill(s[0], a)
        S.put_item(s[0], int(s["agents"]["x"][0, a]), int(s["agents"]["y"][0, a]), Item.PASSAGE)
    return s


def _idle(oracle):
    return _base()


def _rigid(oracle):
    s = _base()
    S.put_item(s[0], 9, 0, Item.RIGID)
    return s


def _bounce(oracle):
    s = _base()
    S.put_item(s[0], 10, 0, Item.PASSAGE)
    S.put_agent(s[0], 2, 0, 1)
    return s


def _bombs(oracle):
    s = _base(2)
    s["agents"]["bombCount"][0, 1] = 1   # agent 1 has its one bomb out (where does not matter to the rule)
    return s


def _pickups(oracle):
    s = _base()
    S.put_item(s[0], 1, 0, Item.EXTRABOMB)
    S.put_item(s[0], 9, 0, Item.INCRRANGE)
    S.put_item(s[0], 9, 10, Item.KICK)
    S.put_item(s[0], 1, 10, Item.KICK)
    s["agents"]["canKick"][0, 3] = 1
    return s


def _expiring_flame(oracle):
    """wood with a hidden incr-range at (1, 0), burnt by a flame of (2, 0) that has one tick left: the flame goes, the item lies there,
    and agent 0 walks onto it, all in the tick under test"""
    s = _base()
    S.put_item(s[0], 1, 0, Item.WOOD + 2)
    oracle.spawn_flame(s, 2, 0, 1)
    for _ in range(S.FLAME_LIFETIME - 1):
        oracle.step(s, IDLE4)
    assert S.is_flame(s["board"][0, 0, 1]), "the flame must still be there when the tick under test begins"
    return s


def _explosions(oracle):
    """agent 0's bomb at (5, 5) and dead agent 1's at (5, 8) both go off, far from everybody (strength 1)"""
    s = _base()
    S.plant_bomb(s[0], 5, 5, 0, True, 1)
    S.plant_bomb(s[0], 5, 8, 1, True, 1)
    S.kill(s[0], 1)
    S.put_item(s[0], 10, 0, Item.PASSAGE)
    return s


def _chain(oracle):
    """agent 0's bomb at (5, 5) goes off and takes agent 1's young one at (6, 5) with it"""
    s = _base()
    S.plant_bomb(s[0], 5, 5, 0, True, 1)
    S.plant_bomb(s[0], 6, 5, 1, True, 7)
    return s


def _walk_into_fire(oracle):
    s = _base()
    oracle.spawn_flame(s, 2, 0, 1)   # (1, 0) burns
    return s


def _blast(oracle):
    """agent 1's bomb at (1, 0) goes off beside agent 0"""
    s = _base()
    S.plant_bomb(s[0], 1, 0, 1, True, 1)
    return s


def _both_die(oracle):
    """agents 2 and 3 are dead; agent 0's bomb at (1, 0) goes off between agent 0 at (0, 0) and agent 1 at (2, 0)"""
    s = _base(2, 3)
    S.put_item(s[0], 10, 0, Item.PASSAGE)
    S.put_agent(s[0], 2, 0, 1)
    S.plant_bomb(s[0], 1, 0, 0, True, 1)
    return s


def _last_opponent(oracle):
    """agents 2 and 3 are dead; agent 0's bomb at (9, 0) goes off beside agent 1"""
    s = _base(2, 3)
    S.plant_bomb(s[0], 9, 0, 0, True, 1)
    return s


def _last_tick(oracle):
    s = _base()
    s["timeStep"][0] = CAP - 1
    return s


def _wood(flagged):
    def build(oracle):
        """agent 0's bomb of strength 2 at (5, 5): wood at (6, 5) and (5, 6) burns, the wood at (7, 5) behind the first is shielded; with
        `flagged` the two that burn hide an extra-bomb and a kick"""
        s = _base()
        s["agents"]["bombStrength"][0, 0] = 2
        S.plant_bomb(s[0], 5, 5, 0, True, 1)
        S.put_item(s[0], 6, 5, Item.WOOD + (1 if flagged else 0))
        S.put_item(s[0], 5, 6, Item.WOOD + (3 if flagged else 0))
        S.put_item(s[0], 7, 5, Item.WOOD)
        return s
    return build


CASES = [
    ("idle", "env", _idle, [(IDLE4, (0x18, 0x18, 0x18, 0x18), 0x1000F, 0)]),
    ("a free move", "env", _idle, [((RIGHT, DOWN, LEFT, UP), (0x5C, 0x5A, 0x5B, 0x59), 0x1000F, 0)]),
    ("blocked by the board's edge and by a wall", "env", _rigid, [((UP, LEFT, IDLE, IDLE), (0x19, 0x1B, 0x18, 0x18), 0x1000F, 0)]),
    ("two agents bounce off one cell", "env", _bounce, [((RIGHT, LEFT, IDLE, IDLE), (0x1C, 0x1B, 0x18, 0x18), 0x1000F, 0)]),
    ("BOMB with ammo, without, and from a dead agent", "env", _bombs, [((BOMB, BOMB, BOMB, IDLE), (0x9D, 0x1D, 0x0D, 0x18), 0x1000B, 0)]),
    ("the three pickups, and a kick for an agent that kicks already", "env", _pickups,
     [((RIGHT, LEFT, LEFT, RIGHT), (0x15C, 0x25B, 0x45B, 0x5C), 0x1000F, 0)]),
    ("a power-up picked up on the tick its flame expires", "env", _expiring_flame, [((RIGHT, IDLE, IDLE, IDLE), (0x25C, 0x18, 0x18, 0x18), 0x1000F, 0)]),
    ("a bomb goes off for a live owner and for a dead one; no wood burns", "env", _explosions,
     [(IDLE4, (0x1018, 0x1008, 0x18, 0x18), 0x1000D, 0)]),
    ("a two-owner chain", "env", _chain, [(IDLE4, (0x1018, 0x1018, 0x18, 0x18), 0x1000F, 0)]),
    ("death by walking into fire", "env", _walk_into_fire, [((RIGHT, IDLE, IDLE, IDLE), (0x2C, 0x18, 0x18, 0x18), 0x1000E, 0)]),
    ("death by blast", "env", _blast, [(IDLE4, (0x28, 0x1018, 0x18, 0x18), 0x1000E, 0)]),
    ("the two last agents die together", "env", _both_die, [(IDLE4, (0x51028, 0x50028, 0x50008, 0x50008), 0x10030, 0)]),
    ("the last opponent dies; the finished env is then not ticked", "env", _last_opponent,
     [(IDLE4, (0x31018, 0x10028, 0x10008, 0x10008), 0x10111, 0), ((RIGHT, BOMB, IDLE, IDLE), (0x10, 0, 0, 0), 0x10111, 0)]),
    ("max_steps reached", "env", _last_tick, [(IDLE4, (0x90018, 0x90018, 0x90018, 0x90018), 0x320005F, 0)]),
    ("two woods burn, one is shielded", "env", _wood(False), [(IDLE4, (0x1018, 0x18, 0x18, 0x18), 0x1000F, 2)]),
    ("woods with hidden items burn", "env", _wood(True), [(IDLE4, (0x1018, 0x18, 0x18, 0x18), 0x1000F, 2)]),
    ("RAW: a free move, no bookkeeping", "raw", _idle, [((RIGHT, IDLE, IDLE, BOMB), (0x5C, 0x18, 0x18, 0x9D), 0xF, 0)]),
    ("RAW: the two last agents die together, nothing ends", "raw", _both_die, [(IDLE4, (0x1028, 0x28, 0x8, 0x8), 0x0, 0), (IDLE4, (0x8, 0x8, 0x8, 0x8), 0x0, 0)]),
]
NAMES = [c[0] for c in CASES]


def group(mode):
    """the cases of one handle"""
    return [c for c in CASES if c[1] == mode]
