"""pom_batch_imagine on the GPU (include/pom_batch.h PomImagineSpec, THE RULE): games built from the agents' view memory of a batch of
SimpleAgent games, byte for byte the numpy checker's (tests/imagine_oracle.py); the round trip through the code-plane export; full
knowledge; the keys of the draws; the distribution of what is drawn; what must not be touched is not; the search calls on the built
envs; the refusals, by name."""
import ctypes as C

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END, PomError, _ImagineSpec
from pomcpp_amd.state import STATE_DTYPE
from tests import imagine_oracle as IO

pytestmark = pytest.mark.gpu
N, TICKS, SEED, BSEED, CAP = 48, 40, 20261020, 11, 200


def _env(n=N, **kw):
    env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=CAP, fresh_boards=True, board_seed=BSEED, **kw)
    env.generate(BSEED)
    return env


class Played:
    """48 envs played 40 ticks by step_mixed(simple = all four), every agent remembering at radius 4 each tick: the handle, its memory
    and viewer_attrs on the device and on the host, and the checker's States and words for every view x samples 0..3 (768 jobs: job
    4 * view + sample).  Made once, shared, never changed: the tests build into `slots`, a second handle."""

    def __init__(self):
        import torch
        self.env, self.slots = _env(), _env()
        self.memory, self.stamp = pa.new_view_memory(N)
        self.attrs = torch.zeros((N, 4, 12), dtype=torch.int32, device="cuda")
        self.full, full_stamp = pa.new_view_memory(N)
        torch.cuda.synchronize()   # (the tensors are torch's, the calls below run on the handle's stream)
        self.env.step_mixed(0, 0, None, 0xF, SEED, 0)   # (allocates the agents' memory)
        for tick in range(TICKS):
            self.env.step_mixed(0, N, None, 0xF, SEED, tick)
            self.env.remember(self.memory, self.stamp, 4, viewer_attrs=self.attrs)
        self.env.remember(self.full, full_stamp, 10)
        self.env.sync()
        self.memory_h, self.attrs_h = self.memory.cpu().numpy(), self.attrs.cpu().numpy()
        self.view, self.sample = np.repeat(np.arange(4 * N), 4), np.tile(np.arange(4), 4 * N)
        self.states, self.words = IO.imagine(self.memory_h, self.attrs_h, self.view, self.sample, SEED)

    def close(self):
        self.env.close()
        self.slots.close()


@pytest.fixture(scope="module")
def played(hip_lib):
    p = Played()
    yield p
    p.close()


def _dev(a, dtype="int32"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _imagine(p, view, sample, first=0, handle=None, **kw):
    """the call into `handle` (p.slots) with the played memory, finished: the words as uint32 on the host"""
    handle = handle or p.slots
    out = handle.imagine(p.memory, p.attrs, _dev(view), first, None if sample is None else _dev(sample), kw.pop("seed", SEED), **kw)
    handle.sync()
    return out.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    if got.tobytes() != want.tobytes():
        for j in range(len(got)):
            for f in STATE_DTYPE.names:
                assert np.array_equal(got[j][f], want[j][f]), f"{what}: job {j}, {f}:\n{got[j][f]}\n{want[j][f]}"


def test_the_played_batch_exercises_the_rule(played):
    p = played
    built = (p.words & IO.BUILT) != 0
    dropped = (p.words & (IO.DROPPED_BOMBS | IO.DROPPED_FLAMES)) != 0
    print(f"built {built.sum()} of {len(p.words)}, with a drop flag {dropped.sum()}, no room {(p.words == IO.NO_ROOM).sum()}")
    assert built.sum() >= 0.9 * len(p.words)
    assert ((p.words >> 8) & 0xFF).max() > 60 and ((p.words >> 16) & 15).any() and p.states["bombs_count"].any() and p.states["flames_count"].any()
    ages = p.memory_h[:, :, 5]
    assert ((ages > 0) & (ages < 255)).any() and (p.memory_h[:, :, 0] >= 10).any()


def test_byte_equality_with_the_checker(played):
    """every view of every env, samples 0..3, 48 jobs a call; a range that starts and ends inside tiles; a shuffled list with "no job"
    entries"""
    p = played
    for k in range(0, len(p.view), N):
        words = _imagine(p, p.view[k:k + N], p.sample[k:k + N])
        assert np.array_equal(words, p.words[k:k + N]), k
        built = (words & IO.BUILT) != 0
        _same(p.slots.get_state()[built], p.states[k:k + N][built], f"jobs {k}..")
    before = p.slots.get_state()
    pick = np.arange(100, 100 + 37) * 5 % len(p.view)
    words = _imagine(p, p.view[pick], p.sample[pick], first=5)
    assert np.array_equal(words, p.words[pick])
    after, built = p.slots.get_state(), (words & IO.BUILT) != 0
    _same(after[5:42][built], p.states[pick][built], "first 5, count 37")
    _same(np.concatenate([after[:5], after[42:], after[5:42][~built]]), np.concatenate([before[:5], before[42:], before[5:42][~built]]), "outside the range")
    rng = np.random.default_rng(7)
    pick = rng.permutation(len(p.view))[:N]
    view, sample = p.view[pick].copy(), p.sample[pick].copy()
    view[[3, 17, 30]] = (-1, 4 * N, -7)
    before = p.slots.get_state()
    words = _imagine(p, view, sample)
    job = (view >= 0) & (view < 4 * N)
    assert np.array_equal(words[job], p.words[pick][job]) and not words[~job].any()
    built = (words & IO.BUILT) != 0
    after = p.slots.get_state()
    _same(after[built], p.states[pick][built], "shuffled")
    _same(after[~built], before[~built], "no job")


def test_round_trip_through_the_code_planes(played):
    """observe(dtype="codes") of an imagined env shows the memory's planes 0..4 on every cell the viewer has seen — but where an agent
    stands that was placed by a draw: the rule's first choice for it are cells the viewer does not see NOW, which it may have seen
    before.  Jobs with a drop flag are left out; they must be at most 1 in 10 (the checker counts 0 of 768 on oracle-played games of
    this shape, tests/test_imagine_host.py)."""
    p = played
    checked = 0
    for k in range(0, len(p.view), N):
        words = _imagine(p, p.view[k:k + N], p.sample[k:k + N])
        codes = p.slots.observe(dtype="codes")[0].cpu().numpy()
        ok = ((words & IO.BUILT) != 0) & ((words & (IO.DROPPED_BOMBS | IO.DROPPED_FLAMES)) == 0)
        views = p.memory_h.reshape(-1, 6, 11, 11)[p.view[k:k + N]]
        seen = (views[:, 5] != 255) & ~IO.drawn_cells(p.slots.get_state(), words)
        bad = np.argwhere((codes != views[:, :5]) & seen[:, None] & ok[:, None, None, None])
        assert bad.size == 0, (k, bad[:5], codes[tuple(bad[0])], views[tuple(bad[0])])
        checked += int(ok.sum())
    assert checked >= 0.9 * len(p.view)


def test_full_knowledge(played):
    """a memory remembered at radius 10: the imagined game has every live agent where it is, the same timeStep and aliveAgents, and
    reach() of it equals reach() of the true env byte for byte, all four agents, both planes"""
    p = played
    true = p.env.get_state()
    want = p.env.reach()
    want = {k: v.cpu().numpy() for k, v in want.items()}
    for v in range(4):
        out = p.slots.imagine(p.full, p.attrs, _dev(np.arange(N) * 4 + v), seed=v)
        p.slots.sync()
        assert (out.cpu().numpy().view(np.uint32) == IO.BUILT).all()   # nothing unknown, nobody drawn, nothing dropped
        got = p.slots.get_state()
        assert np.array_equal(got["timeStep"], true["timeStep"]) and np.array_equal(got["aliveAgents"], true["aliveAgents"])
        assert np.array_equal(got["agents"]["dead"], true["agents"]["dead"])
        alive = true["agents"]["dead"] == 0
        assert np.array_equal(got["agents"]["x"][alive], true["agents"]["x"][alive]) and np.array_equal(got["agents"]["y"][alive], true["agents"]["y"][alive])
        assert np.array_equal(IO.board_codes(got["board"]), IO.board_codes(true["board"]))
        reach = p.slots.reach()
        for k in want:
            assert np.array_equal(reach[k].cpu().numpy(), want[k]), (v, k)


def test_keys(played):
    """the same (view, sample) in two slots and in two calls with different list orders is the same record; samples 0 and 1 of a view
    with unknown cells show the same on every known cell and differ somewhere"""
    p = played
    pick = np.flatnonzero(((p.words >> 8) & 0xFF) >= 30)[:40:2]   # 20 jobs of views with 30 unknown cells or more
    view, sample = np.concatenate([p.view[pick], p.view[pick][::-1]]), np.concatenate([p.sample[pick], p.sample[pick][::-1]])
    words = _imagine(p, view, sample, first=3)
    first = p.slots.get_state(3, 40)
    assert np.array_equal(words[:20], words[39:19:-1]) and (words & IO.BUILT).all()
    _same(first[:20], first[39:19:-1], "two slots")
    order = np.random.default_rng(3).permutation(40)
    assert np.array_equal(_imagine(p, view[order], sample[order], first=8), words[order])
    _same(p.slots.get_state(8, 40), first[order], "another order, other slots")
    views = np.unique(p.view[pick])
    words = _imagine(p, np.repeat(views, 2), np.tile([0, 1], len(views)))
    got = p.slots.get_state(0, 2 * len(views))
    known = IO.known_cells(p.memory_h.reshape(-1, 6, 121).astype(np.int64))[views].reshape(-1, 11, 11)
    codes, free = IO.board_codes(got["board"]), ~IO.drawn_cells(got, words)
    assert np.where(known & free[0::2] & free[1::2], codes[0::2] == codes[1::2], True).all()
    assert (got["board"][0::2] != got["board"][1::2]).any(axis=(1, 2)).all()


def test_distribution_of_the_draws(hip_lib):
    """A wiped view, the viewer alone in a corner, 4,096 samples: 120 unknown cells each.  The counts of passage, rigid and wood over
    them lie within 5 standard deviations of 5/7, 1/7, 1/7 of the cells, the counts of the wood flags within 5 of 1/2 (flag 0) and 1/8
    (each of 1..4) of the woods — binomial: sigma = sqrt(N p (1 - p))."""
    import torch
    samples = 4096
    memory, _ = pa.new_view_memory(1)
    attrs = torch.zeros((1, 4, 12), dtype=torch.int32, device="cuda")
    attrs[0, 2, :8] = torch.tensor([10, 10, 1, 1, 0, 1, 1, 0], dtype=torch.int32)
    with BatchEnvironment(samples, mode=MODE_ENV) as env:
        env.generate(BSEED)
        words = env.imagine(memory, attrs, torch.full((samples,), 2, dtype=torch.int32, device="cuda"), seed=SEED)
        env.sync()
        assert (words.cpu().numpy().view(np.uint32) == IO.BUILT | (121 << 8)).all()
        board = env.get_state()["board"].reshape(samples, 121)[:, :120]   # (the viewer stands on cell 120)
    cells = board.size
    for what, count, share in (("passage", (board == 0).sum(), 5 / 7), ("rigid", (board == 1).sum(), 1 / 7), ("wood", (board >> 8 == 2).sum(), 1 / 7)):
        sigma = np.sqrt(cells * share * (1 - share))
        print(f"{what}: {count} of {cells}, expected {cells * share:.0f}, sigma {sigma:.0f}")
        assert abs(count - cells * share) <= 5 * sigma, what
    assert (board == 0).sum() + (board == 1).sum() + (board >> 8 == 2).sum() == cells
    flags = board[board >> 8 == 2] & 0xFF
    for flag, share in ((0, 1 / 2), (1, 1 / 8), (2, 1 / 8), (3, 1 / 8), (4, 1 / 8)):
        sigma = np.sqrt(flags.size * share * (1 - share))
        print(f"flag {flag}: {(flags == flag).sum()} of {flags.size}, expected {flags.size * share:.0f}, sigma {sigma:.0f}")
        assert abs((flags == flag).sum() - flags.size * share) <= 5 * sigma, flag
    assert flags.max() == 4


def test_what_is_not_built_is_untouched(played):
    """envs outside the range, "no job" and NO_ROOM slots, memory, viewer_attrs, counters, episode counters are as before; the built
    envs have a clear status and fresh agent memory; restore() puts a built env back on the imagined state"""
    import torch
    p = played
    # a 49th env whose view 0 is all walls around the viewer, with a live enemy it has never seen: NO_ROOM
    memory, attrs = torch.cat([p.memory, torch.ones_like(p.memory[:1])]), torch.cat([p.attrs, torch.zeros_like(p.attrs[:1])])
    memory[N, :, 1:] = 0
    attrs[N, 0, :11] = torch.tensor([5, 5, 1, 1, 0, 1, 1, 0, 1, 0, 0], dtype=torch.int32)
    torch.cuda.synchronize()
    memory0, attrs0 = memory.clone(), attrs.clone()
    slots = p.slots
    slots.step_simple(SEED, 3)   # the agents' memory is in use, the games have moved on
    first, count = 5, 37
    pick = np.arange(count) * 13 % len(p.view)
    view, sample = p.view[pick].copy(), p.sample[pick].copy()
    view[[2, 20]], view[[7, 30]] = -1, 4 * N   # no job; NO_ROOM
    before = dict(states=slots.get_state(), status=slots.status(), mem=slots.policy_memory(), counters=slots.counters(), episodes=slots.episodes())
    assert before["mem"].any()
    out = slots.imagine(memory, attrs, _dev(view), first, _dev(sample), SEED)
    slots.sync()
    words = out.cpu().numpy().view(np.uint32)
    want_states, want_words = IO.imagine(memory0.cpu().numpy(), attrs0.cpu().numpy(), view, sample, SEED)
    assert np.array_equal(words, want_words) and (words[[7, 30]] == IO.NO_ROOM).all() and not words[[2, 20]].any()
    built = np.zeros(N, dtype=bool)
    built[first:first + count] = (words & IO.BUILT) != 0
    assert built.sum() >= count - 8
    after = dict(states=slots.get_state(), status=slots.status(), mem=slots.policy_memory(), counters=slots.counters(), episodes=slots.episodes())
    _same(after["states"][first:first + count][built[first:first + count]], want_states[built[first:first + count]], "built")
    _same(after["states"][~built], before["states"][~built], "not built")
    assert np.array_equal(after["mem"][~built], before["mem"][~built]) and not after["mem"][built].any()
    for k in before["status"]:
        assert np.array_equal(after["status"][k][~built], before["status"][k][~built]), k
    assert not after["status"]["done"][built].any() and not after["status"]["ubflags"][built].any()
    assert np.array_equal(after["counters"], before["counters"]) and np.array_equal(after["episodes"], before["episodes"])
    assert torch.equal(memory, memory0) and torch.equal(attrs, attrs0)
    # the restart snapshot of a built env is the imagined state, that of the others what it was
    slots.step_simple(SEED, 2)
    slots.restore(np.flatnonzero(built))
    _same(slots.get_state()[built], after["states"][built], "restored")
    assert not slots.policy_memory()[built].any()


def test_the_handles_tick_is_untouched(hip_lib):
    """step_random's moves are keyed by the handle's tick: a handle that imagined in between plays the tick its twin plays"""
    import torch
    memory, _ = pa.new_view_memory(4)
    attrs = torch.zeros((4, 4, 12), dtype=torch.int32, device="cuda")
    attrs[:, :, 2] = 1
    with _env(32) as a, _env(32) as b:
        for h in (a, b):
            h.step_random(SEED, ticks=3)
        start = a.get_state()
        assert (a.imagine(memory, attrs, _dev(np.arange(16)), first=16, unknown="passage").cpu().numpy() & IO.BUILT).all()
        a.make_game(start[16:], first=16)
        b.make_game(start[16:], first=16)
        for h in (a, b):
            h.step_random(SEED, ticks=2)
        _same(a.get_state(), b.get_state(), "after two more ticks")


def test_chained_into_the_search(played):
    """rollout_jobs and move_safety on the imagined slots equal the same calls on a twin handle into which the checker's States were
    uploaded at the same env indices"""
    import torch
    p = played
    pick = np.arange(N) * 17 % len(p.view)
    words = _imagine(p, p.view[pick], p.sample[pick])
    assert np.array_equal(words, p.words[pick])
    built = (words & IO.BUILT) != 0
    states = p.states[pick].copy()
    states[~built] = p.slots.get_state()[~built]
    src = torch.arange(N, dtype=torch.int64, device="cuda")
    with _env() as twin:
        twin.make_game(states)
        for simple in (0, 0xF):
            got = p.slots.rollout_jobs(src, 24, 3, SEED + 1, simple=simple, fresh_agents=True)
            want = twin.rollout_jobs(src, 24, 3, SEED + 1, simple=simple, fresh_agents=True)
            assert torch.equal(got, want), simple
        got, want = p.slots.move_safety(8), twin.move_safety(8)
        for k in want:
            assert torch.equal(got[k], want[k]), k


def test_refusals(played):
    """ValueError from the wrapper, POM_E_ARG naming the call from the library, and nothing written"""
    import torch
    p = played
    slots = p.slots
    before = slots.get_state()
    view = _dev(np.arange(16))
    for kw in (dict(memory=None), dict(memory=p.memory[:, :, :5]), dict(viewer_attrs=p.attrs[:, :, :8].contiguous()), dict(view=view.to(torch.int64)),
               dict(first=N - 15), dict(first=-1), dict(unknown="fog"), dict(belief=torch.zeros((N, 4, 4), dtype=torch.int32, device="cuda")),
               dict(sample=view[:8]), dict(out=torch.zeros(8, dtype=torch.int32, device="cuda"))):
        args = dict(memory=p.memory, viewer_attrs=p.attrs, view=view)
        args.update(kw)
        with pytest.raises(ValueError):
            slots.imagine(**args)
    out = torch.zeros(16, dtype=torch.int32, device="cuda")

    def refusal(handle=None, **kw):
        fields = dict(unknown=0, first=0, count=16, rows=4 * N, reserved_=0, seed=1, view_dev=view.data_ptr(), sample_dev=None, memory_dev=p.memory.data_ptr(),
                      viewer_attrs_dev=p.attrs.data_ptr(), belief_attrs_dev=None, result_dev=out.data_ptr(), stream=None)
        fields.update(kw)
        size = fields.pop("struct_size", C.sizeof(_ImagineSpec))
        spec = _ImagineSpec(size, *[fields[f] for f, _ in _ImagineSpec._fields_[1:]])
        with pytest.raises(PomError) as e:
            (handle or slots)._call("pom_batch_imagine", C.byref(spec))
        assert e.value.code == 1 and "pom_batch_imagine: " in str(e.value), str(e.value)
        return str(e.value)
    for kw, named in ((dict(view_dev=None), "view_dev is NULL"), (dict(memory_dev=None), "memory_dev is NULL"), (dict(viewer_attrs_dev=None), "viewer_attrs_dev"),
                      (dict(memory_dev=p.memory.data_ptr() + 2), "4-byte"), (dict(view_dev=view.data_ptr() + 1), "4-byte"),
                      (dict(viewer_attrs_dev=p.attrs.data_ptr() + 4), "16-byte"), (dict(struct_size=92), "struct_size"), (dict(rows=4 * N + 2), "rows"),
                      (dict(first=N - 15), "outside the batch"), (dict(first=-1), "outside the batch"), (dict(count=N + 1), "outside the batch"),
                      (dict(unknown=2), "unknown"), (dict(reserved_=7), "reserved_")):
        assert named in refusal(**kw), kw
    with BatchEnvironment(64, lanes_per_env=1, envs_per_wave=64) as one_lane:
        assert "quad" in refusal(one_lane)
    slots.sync()
    _same(slots.get_state(), before, "after the refusals")
    assert not out.any()
