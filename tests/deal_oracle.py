"""TEST INFRASTRUCTURE — THE RULE of pom_batch_deal (include/pom_batch.h PomDealSpec) as a slow, literal Python loop over its clauses, cell
by cell and pair by pair on plain ints: from (seed, env, game, layout) to a 1004-byte State and the result word.  The reference has no
such generator: this checker is the authority for the call.  The draws of include/pom_boardgen.h are restated in a dozen lines; nothing of
the kernel is — no cell sets, no packed numbers, no record: cells are a dict, the flood is a list that grows."""
import numpy as np

from pomcpp_amd.state import STATE_DTYPE, Item, new_states

N = 11
STANDARD = (36, 36, 20, 4, 0)
NO_LANES = 1
DEALT, FALLBACK, ATTEMPTS_SHIFT, BAD_SHIFT = 1, 2, 8, 16
ATTEMPTS = 16
AGENTS = ((1, 1), (9, 1), (9, 9), (1, 9))   # clause 1, (x, y) of agents 0..3
M32 = 0xFFFFFFFF


# ---- include/pom_rng.h, include/pom_boardgen.h on Python ints ----
def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def board_key(seed, env, episode):
    seed, env, episode = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env) & M32, int(episode) & M32
    k = fmix32((episode * 0x7FEB352D + (seed >> 32) + 0x5BD1E995) & M32)
    return fmix32((seed & M32) ^ ((env * 0x9E3779B1) & M32) ^ k)


def board_draw(key, i):
    return fmix32((key + (i + 1) * 0x9E3779B9) & M32)


def below(d, n):
    return (d * n) >> 32


# ---- the layout ----
def lane_woods(layout):
    return 0 if layout[4] & NO_LANES else 12


def layout_ok(layout):
    num_rigid, num_wood, num_items, max_inaccessible, flags = layout
    L = lane_woods(layout)
    return (flags & ~NO_LANES == 0 and num_rigid >= 0 and num_rigid % 2 == 0 and num_wood >= 0 and num_wood % 2 == 0 and num_wood >= L and
            num_rigid // 2 + (num_wood - L) // 2 <= 40 and 0 <= num_items <= num_wood and 0 <= max_inaccessible <= 121)


# ---- clauses 1 - 3 ----
def fixed_cells():
    """{(x, y): "agent0".."agent3" | "passage" | "lane"} of clauses 1 and 2, and the pairs of clause 3 as [((x, y), (y, x))], x > y"""
    fixed = {}
    for a, xy in enumerate(AGENTS):
        fixed[xy] = f"agent{a}"
    for line in (1, 9):
        for pos in range(N):
            kind = "passage" if pos in (2, 3, 7, 8) else "lane" if pos in (4, 5, 6) else None
            if kind:
                fixed[(pos, line)] = kind   # the line y = 1 or y = 9
                fixed[(line, pos)] = kind   # the line x = 1 or x = 9
    for d in range(N):
        fixed.setdefault((d, d), "passage")
    pairs = [((x, y), (y, x)) for y in range(N) for x in range(N) if x > y and (x, y) not in fixed]   # ascending c = y * 11 + x
    assert len(pairs) == 40 and all(lo not in fixed for _, lo in pairs) and len(fixed) + 80 == 121
    return fixed, pairs


FIXED, PAIRS = fixed_cells()


def attempt(key, a, layout):
    """clause 5: {(x, y): "rigid" | "wood" | "passage"} over the 80 pair cells, and the kinds of the 40 pairs in order"""
    need_r, need_w = layout[0] // 2, (layout[1] - lane_woods(layout)) // 2
    cells, kinds = {}, []
    for k, (hi, lo) in enumerate(PAIRS):
        t = below(board_draw(key, 64 * a + k), 40 - k)
        if t < need_r:
            kind, need_r = "rigid", need_r - 1
        elif t < need_r + need_w:
            kind, need_w = "wood", need_w - 1
        else:
            kind = "passage"
        cells[hi] = cells[lo] = kind
        kinds.append(kind)
    return cells, kinds


def whole_board(cells, layout):
    """the 121 cells of an attempt: "rigid" | "wood" | "passage" | "agent<a>" """
    board = dict(cells)
    for xy, kind in FIXED.items():
        board[xy] = ("passage" if layout[4] & NO_LANES else "wood") if kind == "lane" else kind
    assert len(board) == 121
    return board


def inaccessible(board):
    """clause 6: the passage cells that no walk from (1,1) over cells that are not rigid reaches"""
    seen, todo = {(1, 1)}, [(1, 1)]
    while todo:
        x, y = todo.pop()
        for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
            if 0 <= nx < N and 0 <= ny < N and (nx, ny) not in seen and board[(nx, ny)] != "rigid":
                seen.add((nx, ny))
                todo.append((nx, ny))
    return sum(1 for xy, kind in board.items() if kind == "passage" and xy not in seen)


def deal(seed, env, game, layout=STANDARD, env_offset=0):
    """(a State as a STATE_DTYPE array of one, the result word) of board (seed, env_offset + env, game)"""
    assert layout_ok(layout), layout
    key = board_key(seed, env_offset + env, game)
    for a in range(ATTEMPTS):
        board = whole_board(attempt(key, a, layout)[0], layout)
        bad = inaccessible(board)
        if bad <= layout[3]:
            break
    word = DEALT | (FALLBACK if bad > layout[3] else 0) | (a << ATTEMPTS_SHIFT) | (bad << BAD_SHIFT)
    # clause 7
    woods = [y * N + x for y in range(N) for x in range(N) if board[(x, y)] == "wood"]
    left, need, flags = len(woods), layout[2], {}
    for c in woods:
        if below(board_draw(key, 1024 + c), left) < need:
            flags[c] = 1 + below(board_draw(key, 1280 + c), 3)
            need -= 1
        left -= 1
    # clause 8
    s = new_states(1)
    for (x, y), kind in board.items():
        c = y * N + x
        s[0]["board"][y][x] = (Item.PASSAGE if kind == "passage" else Item.RIGID if kind == "rigid" else Item.WOOD + flags.get(c, 0) if kind == "wood"
                               else Item.AGENT0 + int(kind[5]))
    for a, (x, y) in enumerate(AGENTS):
        s[0]["agents"][a]["x"], s[0]["agents"][a]["y"] = x, y
    return s, word


def deal_many(seed, envs, games, layout=STANDARD, env_offset=0):
    """deal() for arrays of envs and games: (STATE_DTYPE [n], uint32 [n])"""
    envs, games = np.asarray(envs).reshape(-1), np.asarray(games).reshape(-1)
    states, words = np.zeros(len(envs), dtype=STATE_DTYPE), np.zeros(len(envs), dtype=np.uint32)
    for j, (e, g) in enumerate(zip(envs.tolist(), games.tolist())):
        s, words[j] = deal(seed, e, g, layout, env_offset)
        states[j] = s[0]
    return states, words


def next_game(g):
    """games[e] after a deal: int32 arithmetic, 2^31 - 1 wraps"""
    return (np.asarray(g).astype(np.int64) + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31
