"""The hand-made cases of pom_batch_imagine (tests/imagine_cases.py) through pom_imagine_kernel itself, in every tile column.  The
host suite runs them through a host loop around the rule functions; what the kernel does around those — the views staged eight at a time
through readlane into LDS, the 2-byte offset of an odd view row, the quad sum of the unknown cells, pom_imagine_finish on a quad's first
lane beside tile-mates that do something else, the put-back of a refused column, the dense snapshot — has only met one played batch, in
which no job drops a bomb or a flame.  Here the cases' one-env memories are stacked into one memory (as listed and reversed, so that both
row 0 and the last row are a case's view), every call of 48 jobs repeats the 13 cases with a rotation (tests/fog_columns.py), and
everything is compared byte for byte with the checker (tests/imagine_oracle.py): words, built States, the cases' own hand-reasoned
`expect`, and the bytes of every slot that is not built."""
import numpy as np
import pytest

from tests import fog_columns as FC
from tests import imagine_cases as IC
from tests import imagine_oracle as IO

CASES = IC.cases()
C = len(CASES)
VIEWS = [c["view"] for c in CASES]
N, SEED, BSEED, CAP = 48, 20261020, 11, 200
ROTATIONS = range(16)
UNKNOWN = {"sample": IO.SAMPLE, "passage": IO.PASSAGE}
gpu = pytest.mark.gpu


# ---- what the placements cover: recounted from the arrays, no GPU ------------------------------------------------------------------
def test_the_rotations_put_every_case_into_every_column():
    FC.check_columns([(FC.jobs(C, r, N), 0) for r in ROTATIONS], C)
    # every call holds every case at least three times, and the short call of test_a_range_with_no_job_entries starts and ends inside tiles
    assert all(np.bincount(FC.jobs(C, r, N), minlength=C).min() >= 3 for r in ROTATIONS)
    assert 5 % 16 and (5 + 37) % 16 and np.bincount(FC.jobs(C, 7, 37), minlength=C).min() >= 2


def test_the_stacked_memory_has_both_parities_and_both_ends():
    rows = [FC.stacked_rows(VIEWS, reverse) for reverse in (False, True)]
    for r in rows:
        assert {int(v) & 1 for v in r} == {0, 1} and len(set(r.tolist())) == C
    assert sum(v & 1 for v in VIEWS) >= 4   # flames_L_and_cross, wiped_viewer_alone and the two clamped cases: the 2-byte LDS offset
    assert 3 in rows[0] and 4 * C - 4 in rows[0] and 4 * C - 1 in rows[1] and 0 in rows[1]   # reversed: row 0 and the memory's last row
    # a call's words hold every kind of outcome side by side (asserted on the device's words too)
    assert {"21_bombs", "21_flame_pieces", "no_room", "bomb_under_an_agent"} <= {c["name"] for c in CASES}


# ---- the GPU ----------------------------------------------------------------------------------------------------------------------
class Stack:
    """the cases' memories, attrs and beliefs stacked along the env axis, on the host and on the device; a case without a belief has
    (1, 1, 0) rows, which the header says equals NULL"""

    def __init__(self, reverse):
        import torch
        order = list(range(C))[::-1] if reverse else list(range(C))
        self.memory = np.concatenate([CASES[i]["memory"] for i in order])
        self.attrs = np.concatenate([CASES[i]["attrs"] for i in order])
        default = np.zeros((1, 4, 4, 3), dtype=np.int32)
        default[..., :2] = 1
        self.belief = np.concatenate([default if CASES[i]["belief"] is None else CASES[i]["belief"] for i in order]).astype(np.int32)
        self.rows = FC.stacked_rows(VIEWS, reverse)
        assert self.memory.shape == (C, 4, 6, 11, 11) and self.attrs.shape == (C, 4, 12) and self.belief.shape == (C, 4, 4, 3)
        for i in range(C):   # the stacking is what stacked_rows says it is
            assert np.array_equal(self.memory.reshape(-1, 6, 11, 11)[self.rows[i]], CASES[i]["memory"][0, VIEWS[i]])
        self.dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (self.memory, self.attrs, self.belief))
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def stacks(hip_lib):
    return {False: Stack(False), True: Stack(True)}


def _env(n=N):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END
    env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=CAP, fresh_boards=True, board_seed=BSEED)
    env.generate(BSEED)
    return env


@pytest.fixture(scope="module")
def slots(hip_lib):
    env = _env()
    yield env
    env.close()


def _same(got, want, what):
    from pomcpp_amd.state import STATE_DTYPE
    if got.tobytes() != want.tobytes():
        for j in range(len(got)):
            for f in STATE_DTYPE.names:
                assert np.array_equal(got[j][f], want[j][f]), f"{what}: entry {j}, {f}:\n{got[j][f]}\n{want[j][f]}"


def _call(env, stack, view, unknown, first=0, sample=None, belief=True, seed=SEED):
    """one call of len(view) jobs into env: the checker's (states, words), the device's words, and every slot before and after"""
    import torch
    before = env.get_state()
    memory, attrs, bel = stack.dev
    out = env.imagine(memory, attrs, torch.from_numpy(np.ascontiguousarray(view, dtype=np.int32)).cuda(), first,
                      None if sample is None else torch.from_numpy(np.ascontiguousarray(sample, dtype=np.int32)).cuda(), seed, unknown,
                      bel if belief else None)
    env.sync()
    words = out.cpu().numpy().view(np.uint32)
    want, want_words = IO.imagine(stack.memory, stack.attrs, view, sample, seed, UNKNOWN[unknown], stack.belief if belief else None)
    return want, want_words, words, before, env.get_state()


def _check(case_of_job, view, unknown, first, want, want_words, words, before, after, what, expect=True):
    """everything the issue asks of one call: the words, every built slot field by field, the cases' own expect on the device's State,
    and every slot that is not built — refused, no job, outside the range — byte for byte as it was"""
    from pomcpp_amd.state import STATE_DTYPE
    count = len(view)
    assert np.array_equal(words, want_words), (what, [hex(w) for w in words], [hex(w) for w in want_words])
    built = np.zeros(len(after), dtype=bool)
    built[first:first + count] = (words & IO.BUILT) != 0
    _same(after[first:first + count][built[first:first + count]], want[built[first:first + count]], what + ": built")
    _same(after[~built], before[~built], what + ": not built")
    for j, i in enumerate(case_of_job):
        if view[j] < 0 or view[j] >= 4 * C:
            assert words[j] == 0, (what, j)
        elif expect and CASES[i]["unknown"] == unknown:
            # (a refused job: the checker's convention is a zero State — the slot's own bytes are compared above)
            state = after[first + j] if words[j] & IO.BUILT else np.zeros((), dtype=STATE_DTYPE)
            CASES[i]["expect"](state, int(words[j]))
    return built


@gpu
@pytest.mark.parametrize("unknown", ["sample", "passage"])
@pytest.mark.parametrize("reverse", [False, True], ids=["listed", "reversed"])
def test_every_case_in_every_column(slots, stacks, reverse, unknown):
    stack = stacks[reverse]
    for r in ROTATIONS:
        case_of_job = FC.jobs(C, r, N)
        view = stack.rows[case_of_job]
        result = _call(slots, stack, view, unknown)
        _check(case_of_job, view, unknown, 0, *result, f"rotation {r}")
        words = result[2]
        # drops and a refusal sit beside ordinary jobs in one wavefront
        assert (words & IO.DROPPED_BOMBS).any() and (words & IO.DROPPED_FLAMES).any() and (words == IO.NO_ROOM).any() and (words == IO.BUILT).any()


@gpu
def test_without_a_belief_and_with_samples_given(slots, stacks):
    """belief = None against the checker's None — bomb_under_an_agent then believes the defaults; sample_dev given: 7 j + 3, and the case's
    number, so that the same (view, sample) is built at columns 13 apart in one call: the same State everywhere"""
    stack = stacks[False]
    case_of_job = FC.jobs(C, 5, N)
    view = stack.rows[case_of_job]
    for unknown in UNKNOWN:
        result = _call(slots, stack, view, unknown, belief=False)
        _check(case_of_job, view, unknown, 0, *result, f"no belief, {unknown}", expect=False)   # (expect was reasoned with the belief)
        with_belief = IO.imagine(stack.memory, stack.attrs, view, None, SEED, UNKNOWN[unknown], stack.belief)[0]
        assert (result[0]["agents"] != with_belief["agents"]).any()   # the belief matters somewhere
        result = _call(slots, stack, view, unknown, sample=7 * np.arange(N) + 3)
        _check(case_of_job, view, unknown, 0, *result, f"samples 7 j + 3, {unknown}")
        result = _call(slots, stack, view, unknown, sample=case_of_job)
        built = _check(case_of_job, view, unknown, 0, *result, f"samples by case, {unknown}")
        after = result[4]
        for i in range(C):
            at = np.flatnonzero((case_of_job == i) & built)
            assert len({int(j) % 16 for j in at}) == len(at) >= (0 if CASES[i]["name"] == "no_room" else 3), (i, at)
            for j in at[1:]:
                _same(after[j:j + 1], after[at[0]:at[0] + 1], f"case {i} at columns {at[0] % 16} and {j % 16}")
                assert result[2][j] == result[2][at[0]]
    # the draws matter: under "sample" two samples of a case with unknown cells differ
    a, _ = IO.imagine(stack.memory, stack.attrs, [stack.rows[0]] * 2, [0, 1], SEED, IO.SAMPLE, stack.belief)
    assert (a[0]["board"] != a[1]["board"]).any()


@gpu
def test_a_range_with_no_job_entries(slots, stacks):
    """first = 5, count = 37, with "no job" entries (-1, rows) in the list: envs 0..4, 42..47 and the no-job slots keep their bytes"""
    first, count = 5, 37
    for reverse, unknown in ((False, "sample"), (True, "passage")):
        stack = stacks[reverse]
        case_of_job = FC.jobs(C, 7, count)
        view = stack.rows[case_of_job].copy()
        view[[2, 20]], view[[9, 30]] = -1, 4 * C
        result = _call(slots, stack, view, unknown, first=first)
        built = _check(case_of_job, view, unknown, first, *result, f"first 5, count 37, {unknown}")
        assert not built[:first].any() and not built[first + count:].any() and not built[[first + 2, first + 20, first + 9, first + 30]].any()
        assert built.sum() >= count - 4 - 4   # all but the no-job entries and the no_room jobs


@gpu
def test_the_snapshot_is_the_record_and_the_agents_are_fresh(stacks):
    """into a handle of its own whose agents have a memory: the built slots' SimpleAgent memory is zero, the others' is as it was; then
    the records are shuffled (copy_envs leaves the snapshots alone) and restore() puts every built slot back on the built State"""
    stack = stacks[True]
    case_of_job = FC.jobs(C, 3, N)
    view = stack.rows[case_of_job]
    with _env() as env:
        env.step_simple(SEED, 3)
        mem0 = env.policy_memory()
        result = _call(env, stack, view, "sample")
        built = _check(case_of_job, view, "sample", 0, *result, "a fresh handle")
        after, mem = result[4], env.policy_memory()
        assert built.any() and not built.all() and mem0[built].any() and mem0[~built].any()
        assert not mem[built].any() and np.array_equal(mem[~built], mem0[~built])
        status = env.status()
        assert not status["done"][built].any() and not status["ubflags"][built].any()
        env.copy_envs(np.roll(np.arange(N), 1))
        assert env.get_state().tobytes() == np.roll(after, 1).tobytes()
        env.restore(np.flatnonzero(built))
        _same(env.get_state()[built], after[built], "restored")
        assert not env.policy_memory()[built].any()
