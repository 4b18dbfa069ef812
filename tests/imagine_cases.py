"""The hand-made cases of pom_batch_imagine (include/pom_batch.h PomImagineSpec, THE RULE): one view each, written cell by cell into a
wiped memory, one or two per clause, with what the rule must build reasoned by hand in `expect(state, word)`.  The view of a case is
row 4 * 0 + v of a memory of one env; the other three rows stay wiped."""
import numpy as np

from pomcpp_amd.state import Item

FOG, NEVER = 5, 255
BUILT, DROPPED_BOMBS, DROPPED_FLAMES, NO_ROOM = 1, 2, 4, 8
A0 = Item.AGENT0


def wiped():
    m = np.zeros((1, 4, 6, 11, 11), dtype=np.uint8)
    m[:, :, 0], m[:, :, 5] = FOG, NEVER
    return m


def seen(m, v, board=0, age=0):
    """the whole of view v seen `age` ticks ago as `board` (passage), nothing on it"""
    m[0, v, 0], m[0, v, 1:5], m[0, v, 5] = board, 0, age
    return m


def put(m, v, x, y, board, strength=0, life=0, direction=0, flame=0, age=0):
    m[0, v, :, y, x] = (board, strength, life, direction, flame, age)


def attrs_of(v, x, y, alive=1, bombs=0, max_bombs=1, strength=1, kick=0, others=(1, 1, 1), t=0):
    """viewer v's row of viewer_attrs (the other rows zero); others: the alive flags of agents v + 1, v + 2, v + 3"""
    a = np.zeros((1, 4, 12), dtype=np.int32)
    a[0, v] = (x, y, alive, max_bombs - bombs, bombs, max_bombs, strength, kick, *others, t)
    return a


def bomb(x, y, owner, strength, time, direction=0):
    return x | (y << 4) | (owner << 8) | (strength << 12) | (time << 16) | (direction << 20)


def _case(name, v, memory, attrs, expect, unknown="passage", belief=None, playable=True):
    return dict(name=name, view=v, memory=memory, attrs=attrs, expect=expect, unknown=unknown, belief=belief, playable=playable)


def cases():
    out = []

    # a wiped view, the viewer alone: all 121 cells are unknown and, asked for passage, passage; the others are dead at (0, 0)
    def wiped_alone(s, w):
        board = np.zeros((11, 11), dtype=np.int64)
        board[10, 0] = A0 + 3
        assert np.array_equal(s["board"], board) and w == BUILT | (121 << 8)
        assert s["aliveAgents"] == 1 and s["timeStep"] == 17 and s["bombs_count"] == 0 and s["flames_count"] == 0
        assert [int(d) for d in s["agents"]["dead"]] == [1, 1, 1, 0]
        assert [(int(a["x"]), int(a["y"])) for a in s["agents"]] == [(0, 0), (0, 0), (0, 0), (0, 10)]
        assert tuple(s["agents"][3])[2:6] == (2, 3, 4, 1) and tuple(s["agents"][0])[2:6] == (0, 1, 1, 0)
    out.append(_case("wiped_viewer_alone", 3, wiped(), attrs_of(3, 0, 10, bombs=2, max_bombs=3, strength=4, kick=1, others=(0, 0, 0), t=17), wiped_alone))

    # a bomb under the viewer and one under an enemy: both show the agent, both are queued, by life; the viewer (bombCount 1) owns the
    # FIRST of the queue, which is the one the enemy stands on, the enemy the other — its bombCount 1, and maxBombCount as believed (3)
    m = seen(wiped(), 0)
    put(m, 0, 5, 5, 10, strength=2, life=7)
    put(m, 0, 3, 3, 11, strength=3, life=4, direction=2, age=2)

    def under_agents(s, w):
        assert w == BUILT and s["board"][5, 5] == A0 and s["board"][3, 3] == A0 + 1 and (s["board"] != 0).sum() == 2
        assert s["bombs_count"] == 2 and s["bombs_index"] == 0
        assert s["bombs_queue"][:3].tolist() == [bomb(3, 3, 0, 3, 4, 2), bomb(5, 5, 1, 2, 7), 0]
        assert tuple(s["agents"][1])[:6] == (3, 3, 1, 3, 2, 1) and tuple(s["agents"][0])[:6] == (5, 5, 1, 1, 1, 0) and s["aliveAgents"] == 2
    belief = np.zeros((1, 4, 4, 3), dtype=np.int32)
    belief[0, 0, 1] = (3, 2, 1)
    out.append(_case("bomb_under_an_agent", 0, m, attrs_of(0, 5, 5, bombs=1, others=(1, 0, 0)), under_agents, belief=belief))

    # 21 bombs on row 0 and row 2, lives 1..10 twice and a 21st of life 10 at the highest cell: that one is dropped and shows passage.
    # The viewer owns none (bombCount 0); agents 1 and 3 live and take turns, agent 1 first: ten bombs each
    m = seen(wiped(), 0)
    for i in range(10):
        put(m, 0, i, 0, 3, strength=1, life=i + 1)
        put(m, 0, i, 2, 3, strength=1, life=i + 1)
    put(m, 0, 10, 2, 3, strength=1, life=10)
    put(m, 0, 9, 9, 11)
    put(m, 0, 1, 9, 13)

    def many_bombs(s, w):
        assert w == BUILT | DROPPED_BOMBS and s["bombs_count"] == 20 and s["board"][2, 10] == 0
        assert (s["board"] == Item.BOMB).sum() == 20
        q = s["bombs_queue"].tolist()
        assert [(b >> 16) & 15 for b in q] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10]
        assert [(b >> 4) & 15 for b in q] == [0, 2] * 10 and [(b >> 8) & 15 for b in q] == [1, 3] * 10
        assert [int(a["bombCount"]) for a in s["agents"]] == [0, 10, 0, 10] and [int(a["maxBombCount"]) for a in s["agents"]] == [1, 10, 1, 10]
    out.append(_case("21_bombs", 0, m, attrs_of(0, 5, 5, others=(1, 0, 1)), many_bombs, playable=False))

    # 21 flame pieces that touch nowhere, lives 1, 2, 3 by turns in cell order: seven of each; the last of life 3 is dropped
    m = seen(wiped(), 0)
    spots = [(x, y) for y in (0, 2, 4, 6) for x in (0, 2, 4, 6, 8, 10)][:21]
    for i, (x, y) in enumerate(spots):
        put(m, 0, x, y, 4, flame=i % 3 + 1)

    def many_flames(s, w):
        assert w == BUILT | DROPPED_FLAMES and s["flames_count"] == 20 and s["flames_index"] == 0
        lx, ly = spots[20]
        assert s["board"][ly, lx] == 0 and (s["board"] >> 16 == 4).sum() == 20
        q = s["flames_queue"]
        assert q["timeLeft"].tolist() == [1] * 7 + [2] * 7 + [3] * 6 and not q["strength"].any()
        assert [(int(f["x"]), int(f["y"])) for f in q[:7]] == spots[0::3]
    out.append(_case("21_flame_pieces", 0, m, attrs_of(0, 5, 9, others=(0, 0, 0)), many_flames, playable=False))

    # an L of life 3 with its corner at (2, 2): one flame, origin the corner, strength 2.  A cross around (7, 7) whose row has life 2 and
    # whose column ends have life 1: (7, 6) alone, then the row from (6, 7), strength 2, then (7, 8) alone.  Queue: by life, then origin
    m = seen(wiped(), 1)
    for x, y in ((2, 2), (3, 2), (4, 2), (2, 3), (2, 4)):
        put(m, 1, x, y, 4, flame=3)
    for x, y, life in ((7, 6, 1), (6, 7, 2), (7, 7, 2), (8, 7, 2), (7, 8, 1)):
        put(m, 1, x, y, 4, flame=life)

    def shapes(s, w):
        assert w == BUILT and s["flames_count"] == 4
        assert [tuple(int(k) for k in f) for f in s["flames_queue"][:5]] == [(7, 6, 1, 0), (7, 8, 1, 0), (6, 7, 2, 2), (2, 2, 3, 2), (0, 0, 0, 0)]
        ids = {(x, y): (int(s["board"][y, x]) - Item.FLAMES) >> 3 for y in range(11) for x in range(11) if s["board"][y, x] >> 16 == 4}
        assert ids == {(2, 2): 24, (3, 2): 24, (4, 2): 24, (2, 3): 24, (2, 4): 24, (7, 6): 73, (6, 7): 83, (7, 7): 83, (8, 7): 83, (7, 8): 95}
        assert all((int(s["board"][y, x]) & 7) == 0 for x, y in ids)
    out.append(_case("flames_L_and_cross", 1, m, attrs_of(1, 0, 0, others=(0, 0, 0)), shapes))

    # a dead viewer: dead where it died, its remembered code is passage; the live enemy it remembers stands where it was seen
    m = seen(wiped(), 2, age=3)
    put(m, 2, 4, 4, 12, age=3)
    put(m, 2, 6, 1, 10, age=9)

    def dead_viewer(s, w):
        assert w == BUILT and s["board"][4, 4] == 0 and s["board"][1, 6] == A0 and (s["board"] != 0).sum() == 1
        assert tuple(s["agents"][2])[:2] == (4, 4) and [int(d) for d in s["agents"]["dead"]] == [0, 1, 1, 1] and s["aliveAgents"] == 1
    out.append(_case("dead_viewer", 2, m, attrs_of(2, 4, 4, alive=0, others=(0, 1, 0)), dead_viewer))

    # a dead enemy's stale code on a bomb that still ticks: the cell shows the bomb, which is the viewer's (nobody else lives)
    m = seen(wiped(), 0)
    put(m, 0, 8, 8, 12, strength=2, life=5, age=6)
    put(m, 0, 1, 1, 13, age=6)

    def stale_dead(s, w):
        assert w == BUILT and s["board"][8, 8] == Item.BOMB and s["board"][1, 1] == 0 and s["bombs_queue"][0] == bomb(8, 8, 0, 2, 5)
        assert [int(d) for d in s["agents"]["dead"]] == [0, 1, 1, 1] and tuple(s["agents"][2])[:3] == (0, 0, 0)
    out.append(_case("dead_enemys_stale_code", 0, m, attrs_of(0, 5, 5, others=(0, 0, 0)), stale_dead))

    # an unseen live enemy and no passage anywhere: refused
    m = seen(wiped(), 0, board=1)
    put(m, 0, 5, 5, 10)
    def no_room(s, w):
        assert w == NO_ROOM and not s["board"].any() and s["aliveAgents"] == 0   # (the checker leaves the State of a refused job zero)
    out.append(_case("no_room", 0, m, attrs_of(0, 5, 5, others=(1, 0, 0)), no_room, playable=False))

    # garbage on known cells (9, fog seen "now", 77): unknown cells, passage when asked for passage, and the word counts three
    m = seen(wiped(), 0, board=1)
    for x, b in ((1, 9), (2, 5), (3, 77)):
        put(m, 0, x, 0, b)

    def garbage(s, w):
        assert w == BUILT | (3 << 8) and s["board"][0, :5].tolist() == [1, 0, 0, 0, 1]
    out.append(_case("garbage_byte_on_a_known_cell", 0, m, attrs_of(0, 5, 5, others=(0, 0, 0)), garbage))

    # bytes beyond what a record holds (clauses 1, 4, 5).  Four bombs on row 0: (8, 0) is an ordinary one and leads the queue by its life 9;
    # the others have life 40, 16, 255 -> time 15, strength 200, 16 -> 15 (3 stays), direction 7, 5 -> 0 (4 stays), in cell order.  The viewer's
    # bombCount 300 is more than there are bombs: all four are its own, and it is stored as 107.  Flame bytes 200, 127, 128 are all life 127:
    # (1, 3) and (2, 3) are one flame of strength 1, (4, 3) behind the gap another.  A life byte on wood, passage, a power-up and a burnt-out
    # flame (fl 0) makes no bomb: the cells are what their board byte says
    m = seen(wiped(), 1)
    put(m, 1, 2, 0, 3, strength=200, life=40, direction=7)
    put(m, 1, 4, 0, 3, strength=16, life=16, direction=4)
    put(m, 1, 6, 0, 3, strength=3, life=255, direction=5)
    put(m, 1, 8, 0, 3, strength=2, life=9, direction=2)
    put(m, 1, 1, 3, 4, flame=200)
    put(m, 1, 2, 3, 4, flame=127)
    put(m, 1, 4, 3, 4, flame=128)
    put(m, 1, 3, 6, 2, strength=5, life=9)
    put(m, 1, 5, 6, 0, life=7)
    put(m, 1, 7, 6, 6, life=3)
    put(m, 1, 9, 6, 4, life=5)
    put(m, 1, 9, 9, 13)

    def clamped_bombs(s, w):
        assert w == BUILT and s["bombs_count"] == 4 and s["bombs_index"] == 0
        assert s["bombs_queue"][:5].tolist() == [bomb(8, 0, 1, 2, 9, 2), bomb(2, 0, 1, 15, 15), bomb(4, 0, 1, 15, 15, 4), bomb(6, 0, 1, 3, 15), 0]
        assert s["board"][0].tolist() == [0, 0, Item.BOMB, 0, Item.BOMB, 0, Item.BOMB, 0, Item.BOMB, 0, 0]
        assert s["flames_count"] == 2 and s["flames_index"] == 0
        assert [tuple(int(k) for k in f) for f in s["flames_queue"][:3]] == [(1, 3, 127, 1), (4, 3, 127, 0), (0, 0, 0, 0)]
        assert s["board"][3].tolist() == [0, Item.FLAMES + (34 << 3), Item.FLAMES + (34 << 3), 0, Item.FLAMES + (37 << 3), 0, 0, 0, 0, 0, 0]
        assert s["board"][6, 3] >> 8 == 2 and s["board"][6, 5] == 0 and s["board"][6, 7] == 6 and s["board"][6, 9] == 0
        assert s["board"][5, 5] == A0 + 1 and s["board"][9, 9] == A0 + 3 and (s["board"] != 0).sum() == 4 + 3 + 2 + 2
        assert tuple(s["agents"][1])[:6] == (5, 5, 107, 2, 1, 0) and tuple(s["agents"][3])[:6] == (9, 9, 0, 1, 1, 0) and s["aliveAgents"] == 2
    out.append(_case("clamped_bombs_and_flames", 1, m, attrs_of(1, 5, 5, bombs=300, max_bombs=2, others=(0, 1, 0)), clamped_bombs))

    # a viewer row beyond the board and the record (clauses 4, 6): (-3, 14) is (0, 10); bombCount -500 is stored as -108 and owns nothing — the
    # one bomb goes to agent 0, the only other one alive —, maxBombCount 40000 is 32646, bombStrength 200 is 134, canKick 7 is 1.  (One row
    # holds one bombCount: the count larger than the bombs is clamped_bombs_and_flames'.)  The viewer's own code where it no longer stands
    # places nobody: passage
    m = seen(wiped(), 3)
    put(m, 3, 4, 4, 10, age=2)
    put(m, 3, 7, 7, 3, strength=2, life=6)
    put(m, 3, 2, 2, 13, age=5)

    def clamped_viewer(s, w):
        assert w == BUILT and s["board"][10, 0] == A0 + 3 and s["board"][4, 4] == A0 and s["board"][7, 7] == Item.BOMB and s["board"][2, 2] == 0
        assert (s["board"] != 0).sum() == 3 and s["bombs_count"] == 1 and s["bombs_queue"][:2].tolist() == [bomb(7, 7, 0, 2, 6), 0]
        assert tuple(s["agents"][3])[:6] == (0, 10, -108, 32646, 134, 1) and tuple(s["agents"][0])[:6] == (4, 4, 1, 1, 1, 0)
        assert [int(d) for d in s["agents"]["dead"]] == [0, 1, 1, 0] and s["aliveAgents"] == 2 and s["timeStep"] == 799 and s["flames_count"] == 0
    out.append(_case("clamped_viewer_attrs", 3, m, attrs_of(3, -3, 14, bombs=-500, max_bombs=40000, strength=200, kick=7, others=(1, 0, 0), t=799),
                     clamped_viewer))

    # an unseen enemy goes to a cell the viewer does not see NOW: three stale passage cells among cells seen this tick — and to any
    # passage cell when every cell is seen now
    m = seen(wiped(), 0)
    for x in (3, 6, 9):
        put(m, 0, x, 7, 0, age=4)

    def unseen_cells(s, w):
        assert w == BUILT | (1 << 17) and int(s["agents"][1]["y"]) == 7 and int(s["agents"][1]["x"]) in (3, 6, 9)
        assert s["board"][7, int(s["agents"][1]["x"])] == A0 + 1
    out.append(_case("unseen_enemy_where_the_viewer_does_not_look", 0, m, attrs_of(0, 5, 5, others=(1, 0, 0)), unseen_cells))

    def anywhere(s, w):
        x, y = int(s["agents"][3]["x"]), int(s["agents"][3]["y"])
        assert w == BUILT | (1 << 19) and s["board"][y, x] == A0 + 3 and (x, y) != (5, 5)
    out.append(_case("unseen_enemy_all_seen", 0, seen(wiped(), 0), attrs_of(0, 5, 5, others=(0, 0, 1)), anywhere))
    return out
