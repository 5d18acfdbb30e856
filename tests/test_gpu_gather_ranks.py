"""cilqr_gather_results (cilqr_amd/csrc/comm.hip) with MORE THAN ONE rank, over the loopback transport
(cilqr_comm_create_loopback, include/cilqr.h "test hooks"): W handles of this process on device 0, one Python thread per
rank (ctypes releases the GIL during the call), every thread joined within a bound.

Inputs are crafted.  Trajectory rows are genuine device exports -- one small solved batch, cut and rolled into every rank's
`local->traj` -- so the `time` and `kappa` columns the root rebuilds are comparable bit for bit.  cost_hist, n_cost, status
and n_iter are synthetic: a distinct bit pattern per (rank, problem, row, field), so that any misplacement shows.
The reference is plain NumPy: the locals concatenated in rank order; cost_hist rows below n_cost equal the locals', rows at or
above n_cost keep their sentinel.  Every comparison is array_equal on bits.  Every `gathered` array sits inside a larger
sentinel-filled tensor whose guard bands are checked, non-root ranks pass gathered = NULL, every `local` is unchanged.

What the loopback cannot see (the order of work BETWEEN streams that RCCL relies on) is stated in DESIGN section 7."""
import itertools
import threading
import time

import numpy as np
import pytest

from cilqr_amd import api, scenario

pytestmark = pytest.mark.gpu

TIMEOUT_MS = 20000          # the bound of every wait of the transport (the figure PeerGather uses, tests/test_host.py)
JOIN_S = 90.0               # the bound of every thread: several waits of the transport, never reached by a passing test
SENT = -7                   # sentinel of `gathered` and of its guard bands
DEAD = -3.0                 # local cost_hist rows at or above n_cost: must not travel
GUARD = 1024                # elements on either side of a gathered array
MAX_ITER = 40               # M1 = 41 > 32: the message region (32 rows per problem) is smaller than a dense history
_GROUP = itertools.count(0x6C6F6F70_0000)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def solved():
    """[300][K][10] trajectory rows as the device exports them (mix11, N = 50); read-only, shared by every test."""
    sc = scenario.generate("mix11", 300, seed=170)
    opt = api.BatchIlqrOptimizer(api.default_config(sc["n_steps"]), batch_capacity=300, cmax=sc["cmax"])
    traj = opt.plan(sc)["traj"].copy()
    opt.close()
    assert traj.shape == (300, sc["n_steps"] + 1, 10) and sc["n_steps"] == 50
    assert np.isfinite(traj).all() and len(np.unique(traj[:, -1, 1])) > 250      # rows differ: a misplaced row shows
    traj.flags.writeable = False
    return traj


@pytest.fixture(scope="module")
def handles():
    """Eight handles with M1 = 41 and three with M1 = 6.  The gather reads a handle's configuration and stream only, so
    a capacity of one problem will do; every test puts communicators of its own on them."""
    made = {m: [api.BatchIlqrOptimizer(api.default_config(50, max_iter=m), batch_capacity=1) for _ in range(n)]
            for m, n in ((MAX_ITER, 8), (5, 3))}
    yield made
    for opts in made.values():
        for o in opts:
            o.close()


class World:
    """A loopback communicator over the first W handles."""

    def __init__(self, opts, W, timeout_ms=TIMEOUT_MS):
        self.opts, self.W = opts[:W], W
        self.M1 = opts[0].cfg.max_iter + 1
        group = next(_GROUP)
        for r, o in enumerate(self.opts):
            o.comm_create_loopback(group, r, W, timeout_ms)

    def close(self):
        for o in self.opts:
            assert o.L.cilqr_comm_destroy(o.h) == api.OK

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def gather(self, batches, locs, root, gat, bound=JOIN_S):
        """One cilqr_gather_results per rank, each on a thread of its own -> (return codes, seconds of the slowest)."""
        rc, secs = [None] * self.W, [None] * self.W

        def rank(r):
            t0 = time.monotonic()
            rc[r] = self.opts[r].gather_results_raw(batches[r], locs[r].sol(), root, gat.sol() if r == root else None)
            secs[r] = time.monotonic() - t0

        threads = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(self.W)]
        for t in threads:
            t.start()
        end = time.monotonic() + bound
        for t in threads:
            t.join(max(0.0, end - time.monotonic()))
        assert not any(t.is_alive() for t in threads), "a rank is still inside cilqr_gather_results"
        assert None not in rc
        return rc, max(secs)


def hist_bits(r, B, M1):
    """[B][M1][5] doubles in [1, 2), every one with bits of its own: rank, problem, row and field in the mantissa."""
    b, m, e = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(M1, dtype=np.uint64), np.arange(5, dtype=np.uint64), indexing="ij")
    bits = np.uint64(0x3FF0000000000000) | (np.uint64(r + 1) << np.uint64(44)) | (b << np.uint64(24)) | (m << np.uint64(8)) | (e + np.uint64(1))
    return bits.view(np.float64)


class Local:
    """A rank's results: host originals and their device copies."""

    def __init__(self, torch, solved, r, B, M1, n_cost, with_n_iter=True, roll=0):
        n_cost = np.asarray(n_cost, np.int32)
        assert n_cost.shape == (B,) and n_cost.min() >= 0 and n_cost.max() <= M1
        rows = (r * 101 + 3 * np.arange(B) + 17 + roll) % len(solved)          # cut and rolled; cyclic for B > 300
        hist = hist_bits(r, B, M1)
        hist[np.arange(M1)[None, :] >= n_cost[:, None]] = DEAD
        self.np = dict(traj=np.ascontiguousarray(solved[rows]), hist=hist, nc=n_cost,
                       st=((r + 1) * 10_000_000 + np.arange(B)).astype(np.int32),
                       ni=(-(r + 1) * 10_000_000 - np.arange(B)).astype(np.int32))
        self.dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in self.np.items()}
        self.with_n_iter = with_n_iter

    def sol(self):
        d = self.dev
        return api.SolutionBatch(api.MEM_DEVICE, 0, d["traj"].data_ptr(), d["hist"].data_ptr(), d["nc"].data_ptr(),
                                 d["st"].data_ptr(), d["ni"].data_ptr() if self.with_n_iter else None, None, None)

    def assert_unchanged(self):
        for k, v in self.np.items():
            assert np.array_equal(self.dev[k].cpu().numpy().view(np.int32), v.view(np.int32)), k


class Gathered:
    """The root's destination: every array an interior slice of a larger tensor full of the sentinel."""

    def __init__(self, torch, n, K, M1, with_n_iter=True):
        self.torch, self.n = torch, n
        shapes = dict(traj=((n, K, 10), torch.float64), hist=((n, M1, 5), torch.float64), nc=((n,), torch.int32),
                      st=((n,), torch.int32), ni=((n,), torch.int32))
        self.base, self.view = {}, {}
        for k, (shape, dt) in shapes.items():
            count = int(np.prod(shape))
            self.base[k] = torch.full((count + 2 * GUARD,), SENT, dtype=dt, device="cuda:0")
            self.view[k] = self.base[k][GUARD:GUARD + count].view(shape)
            assert self.view[k].data_ptr() == self.base[k].data_ptr() + GUARD * self.base[k].element_size()
        self.with_n_iter = with_n_iter

    def sol(self):
        v = self.view
        return api.SolutionBatch(api.MEM_DEVICE, 0, v["traj"].data_ptr(), v["hist"].data_ptr(), v["nc"].data_ptr(),
                                 v["st"].data_ptr(), v["ni"].data_ptr() if self.with_n_iter else None, None, None)

    def host(self, k):
        return self.view[k].cpu().numpy()

    def assert_guards(self):
        for k, b in self.base.items():
            count = b.numel() - 2 * GUARD
            assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + count:] == SENT).all()), f"guard band of {k}"

    def assert_untouched(self):
        self.assert_guards()
        for k, b in self.base.items():
            assert bool((b == SENT).all()), k

    def refill(self):
        for b in self.base.values():
            b.fill_(SENT)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def assert_gathered(gat, locs, M1, local_n_iter=True):
    """`gathered` against the locals in rank order, bit for bit; guard bands intact; locals unchanged."""
    gat.assert_guards()
    assert same_bits(gat.host("traj"), np.concatenate([l.np["traj"] for l in locs]))
    n_cost = np.concatenate([l.np["nc"] for l in locs])
    assert same_bits(gat.host("nc"), n_cost)
    assert same_bits(gat.host("st"), np.concatenate([l.np["st"] for l in locs]))
    if gat.with_n_iter:
        ni = np.concatenate([l.np["ni"] for l in locs])
        assert same_bits(gat.host("ni"), ni if local_n_iter else np.zeros_like(ni))
    else:
        assert bool((gat.base["ni"] == SENT).all())
    live = np.arange(M1)[None, :] < n_cost[:, None]
    hist, ref = gat.host("hist"), np.concatenate([l.np["hist"] for l in locs])
    assert same_bits(hist[live], ref[live])
    assert bool((hist[~live] == SENT).all())                  # rows at or above n_cost keep their sentinel
    for l in locs:
        l.assert_unchanged()


def run(torch, solved, world, B, n_costs, root, gat=None, with_n_iter=True, local_n_iter=True, roll=0):
    """One gather of crafted locals (n_costs[r]: rank r's n_cost) held against the reference."""
    K, M1 = solved.shape[1], world.M1
    locs = [Local(torch, solved, r, B, M1, n_costs[r], with_n_iter=local_n_iter, roll=roll) for r in range(world.W)]
    gat = gat or Gathered(torch, world.W * B, K, M1, with_n_iter=with_n_iter)
    torch.cuda.synchronize()
    rc, _ = world.gather([B] * world.W, locs, root, gat)
    torch.cuda.synchronize()
    assert rc == [api.OK] * world.W, rc
    assert_gathered(gat, locs, M1, local_n_iter=local_n_iter)
    return locs, gat


def totals(n_costs):
    return [int(np.sum(n, dtype=np.int64)) for n in n_costs]


def boundary_inside_a_problem(n_cost, cap):
    """The window boundary `cap` of a rank's packed row sequence cuts one problem's rows in two."""
    off = np.concatenate([[0], np.cumsum(n_cost, dtype=np.int64)])
    return bool(((off[:-1] < cap) & (cap < off[1:])).any())


# ---------------------------------------------------------------------------------------------------------------------
# 1. placement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,root", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (8, 0), (8, 7)])
@pytest.mark.parametrize("B", [1, 37, 300])
def test_every_rank_lands_in_its_own_block(torch, solved, handles, W, root, B):
    """Blocks on both sides of the root (slot_of), one problem per rank, a batch that is no multiple of anything, more
    than one block of the pack kernels.  Rank 1 has no live rows at all; a problem of rank 0 has all M1 of them (B > 1: with
    one problem that alone would exceed the region).  No rank exceeds the region: one exchange."""
    with World(handles[MAX_ITER], W) as world:
        M1, cap = world.M1, 32 * B
        assert M1 > 32
        n_costs = [(5 * np.arange(B) + 3 * r + 1) % 21 for r in range(W)]
        n_costs[1] = np.zeros(B, np.int64)
        if B > 1:
            n_costs[0][B // 2] = M1
        assert all(t <= cap for t in totals(n_costs)) and totals(n_costs)[0] > 0
        run(torch, solved, world, B, n_costs, root)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the region's edge: cap = 32 B live rows travel in the message, the rest in a second exchange
# ---------------------------------------------------------------------------------------------------------------------
def _edge_patterns(W, B, M1, root):
    cap, other = 32 * B, (root + 1) % W
    small = [(3 * np.arange(B) + r) % 9 for r in range(W)]
    full = np.full(B, 32, np.int64)
    plus1 = full.copy()
    plus1[B // 3] = 33
    pats = {}
    pats["exactly_cap_on_a_non_root"] = ([full if r == other else small[r] for r in range(W)], [])
    pats["cap_plus_1_on_a_non_root_only"] = ([plus1 if r == other else small[r] for r in range(W)], [other])
    pats["cap_plus_1_on_the_root_only"] = ([plus1 if r == root else small[r] for r in range(W)], [root])
    over = []
    for r in range(W):
        n = full.copy()
        n[: 2 * r + 1] = 33 + 2 * r                       # over by (2 r + 1)^2: another amount on every rank
        over.append(n)
    pats["every_rank_over_by_another_amount"] = (over, list(range(W)))
    pats["all_rows_live_on_one_rank"] = ([np.full(B, M1, np.int64) if r == other else small[r] for r in range(W)], [other])
    pats["all_rows_live_on_the_root_and_cap_plus_1_beside_it"] = (
        [np.full(B, M1, np.int64) if r == root else plus1 if r == other else small[r] for r in range(W)], [root, other])
    return cap, pats


EDGES = ["exactly_cap_on_a_non_root", "cap_plus_1_on_a_non_root_only", "cap_plus_1_on_the_root_only",
         "every_rank_over_by_another_amount", "all_rows_live_on_one_rank", "all_rows_live_on_the_root_and_cap_plus_1_beside_it"]


@pytest.mark.parametrize("root", [0, 1, 2])
@pytest.mark.parametrize("edge", EDGES)
def test_rows_at_the_edge_of_the_message_region(torch, solved, handles, edge, root):
    """W = 3, B = 37.  Ranks with and without rows beyond the region in the same exchange; the root in front, in the middle
    and at the end (the at[] prefix sums over ranks, the root's own window packed at at[root])."""
    W, B = 3, 37
    with World(handles[MAX_ITER], W) as world:
        cap, pats = _edge_patterns(W, B, world.M1, root)
        n_costs, over = pats[edge]
        tot = totals(n_costs)
        assert [r for r in range(W) if tot[r] > cap] == sorted(over)
        if edge == "exactly_cap_on_a_non_root":
            assert max(tot) == cap
        if edge.startswith("cap_plus_1"):
            assert tot[over[0]] == cap + 1
        if edge == "every_rank_over_by_another_amount":
            assert len({t - cap for t in tot}) == W
        if "all_rows_live" in edge:
            assert max(tot) == B * world.M1
        for r in over:                       # the window [cap, total) starts inside one problem's rows
            if tot[r] < B * world.M1 or world.M1 * (cap // world.M1) != cap:
                assert boundary_inside_a_problem(n_costs[r], cap), (edge, r)
        run(torch, solved, world, B, n_costs, root)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a dense history smaller than the region
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("root", [0, 1])
def test_a_history_shorter_than_the_region(torch, solved, handles, root):
    """max_iter = 5: M1 = 6 < 32, cap = B M1, every row fits the message even with all of them live."""
    W, B = 3, 37
    with World(handles[5], W) as world:
        assert world.M1 == 6
        n_costs = [(np.arange(B) + 3) % 7, np.full(B, 6, np.int64), (5 * np.arange(B)) % 7]
        assert totals(n_costs)[1] == B * world.M1
        run(torch, solved, world, B, n_costs, root)


# ---------------------------------------------------------------------------------------------------------------------
# 4. k_row_offsets with more than one row per thread
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,per", [(1025, 2), (2049, 3)])
def test_row_offsets_of_batches_beyond_one_problem_per_thread(torch, solved, handles, B, per):
    """The prefix sum is one block of 1024 threads: `per` problems per thread, the last threads empty.  Rank 1 exceeds the
    region, so the offsets also place the second window."""
    assert (B + 1023) // 1024 == per and per * 1023 >= B      # thread 1023 holds nothing
    with World(handles[MAX_ITER], 2) as world:
        n_costs = [(7 * np.arange(B)) % 23, 31 + (np.arange(B) % 4)]
        assert totals(n_costs)[0] <= 32 * B < totals(n_costs)[1]
        assert boundary_inside_a_problem(n_costs[1], 32 * B)
        run(torch, solved, world, B, n_costs, root=0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. one communicator, several gathers
# ---------------------------------------------------------------------------------------------------------------------
def test_one_communicator_through_moving_roots_and_batches(torch, solved, handles):
    """The root moves 0 -> W - 1 -> 0 (the new root's receive buffer grows from nothing); all ranks move to a smaller and
    then to a larger batch (the agreement runs again, the staging grows); the same gather twice gives the same output."""
    W = 3
    with World(handles[MAX_ITER], W) as world:
        def n_costs(B, k):
            return [(3 * np.arange(B) + r + k) % 40 for r in range(W)]       # about 19.5 a problem: below the region
        for k, (B, root) in enumerate([(37, 0), (37, W - 1), (37, 0), (5, 0), (64, 1), (64, 0)]):
            run(torch, solved, world, B, n_costs(B, k), root, roll=k)
        # twice the same, into the same destination: the second run leaves exactly the first one's bytes
        B, K = 64, solved.shape[1]
        locs = [Local(torch, solved, r, B, world.M1, n_costs(B, 9)[r]) for r in range(W)]
        gat = Gathered(torch, W * B, K, world.M1)
        torch.cuda.synchronize()
        seen = []
        for _ in range(2):
            rc, _ = world.gather([B] * W, locs, 2, gat)
            torch.cuda.synchronize()
            assert rc == [api.OK] * W
            assert_gathered(gat, locs, world.M1)
            seen.append({k: b.cpu().numpy().copy() for k, b in gat.base.items()})
        for k in seen[0]:
            assert same_bits(seen[0][k], seen[1][k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. n_iter is optional on both sides
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["gathered", "local"])
def test_n_iter_left_out(torch, solved, handles, where):
    """gathered->n_iter = NULL: nothing is written for it.  local->n_iter = NULL on every rank: the gathered values are zeros."""
    W, B = 3, 37
    with World(handles[MAX_ITER], W) as world:
        n_costs = [(3 * np.arange(B) + r) % 30 for r in range(W)]
        run(torch, solved, world, B, n_costs, root=1, with_n_iter=where != "gathered", local_n_iter=where != "local")


# ---------------------------------------------------------------------------------------------------------------------
# 7. ranks that do not hold the same batch, where every rank takes part in the agreement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [2, 0])
def test_batch_mismatch_where_every_rank_takes_part_in_the_agreement(torch, solved, handles, odd):
    """W = 3, root 0; the odd rank a non-root, then the root itself.  At a communicator's first gather every rank takes part
    in the agreement: CILQR_ERR_ARG on every rank, nothing written to `gathered`.  A gather with equal batches on the same
    communicator then succeeds; so does the mismatch again when all ranks have moved away from the agreed batch."""
    W, B, root = 3, 37, 0
    K = solved.shape[1]
    with World(handles[MAX_ITER], W) as world:
        M1 = world.M1
        for step in ((20, B), None, (9, 12)):
            if step is None:                                    # equal batches in between: correct, and agreed on
                run(torch, solved, world, B, [(3 * np.arange(B) + r) % 30 for r in range(W)], root)
                continue
            first, others = step
            batches = [first if r == odd else others for r in range(W)]
            locs = [Local(torch, solved, r, batches[r], M1, (np.arange(batches[r]) + r) % 30) for r in range(W)]
            gat = Gathered(torch, W * batches[root], K, M1)
            torch.cuda.synchronize()
            rc, secs = world.gather(batches, locs, root, gat)
            torch.cuda.synchronize()
            assert rc == [api.ERR_ARG] * W, rc
            assert secs < TIMEOUT_MS / 1000.0 / 2               # a verdict, not a wait that ran out
            gat.assert_untouched()
            for l in locs:
                l.assert_unchanged()


# ---------------------------------------------------------------------------------------------------------------------
# 8. one rank alone changes its batch after an agreed gather: outside what the library checks
# ---------------------------------------------------------------------------------------------------------------------
def test_one_rank_alone_changing_its_batch_is_not_an_agreement(torch, solved, handles):
    """include/cilqr.h: the batch is checked where every rank takes part in the check; one rank that alone changes its batch
    breaks a precondition.  What happens then, pinned on the loopback: the offender posts the 8-byte agreement against the
    root's receive of a full message; the pair fails at the rendezvous on both sides -- CILQR_ERR_DEVICE on the root and on
    the offender, NOT CILQR_ERR_ARG on every rank -- well inside the bound; the third rank's message is complete, so it returns
    CILQR_OK; nothing is written to `gathered`, so nothing reports OK for a foreign batch.  (Under RCCL the same pair is a send
    and a receive of different sizes: undefined.)  Back on the agreed batch the communicator works again."""
    W, B, root, offender, timeout_ms = 3, 37, 0, 2, 1500
    K = solved.shape[1]
    with World(handles[MAX_ITER], W, timeout_ms=timeout_ms) as world:
        M1 = world.M1
        n_costs = [(3 * np.arange(B) + r) % 30 for r in range(W)]
        run(torch, solved, world, B, n_costs, root)
        batches = [20 if r == offender else B for r in range(W)]
        locs = [Local(torch, solved, r, batches[r], M1, (np.arange(batches[r]) + r) % 30) for r in range(W)]
        gat = Gathered(torch, W * B, K, M1)
        torch.cuda.synchronize()
        rc, secs = world.gather(batches, locs, root, gat, bound=10 * timeout_ms / 1000.0)
        torch.cuda.synchronize()
        assert rc[root] != api.OK and rc[offender] != api.OK, rc                 # required whatever else happens
        assert rc == [api.ERR_DEVICE, api.OK, api.ERR_DEVICE], rc                # what the code does
        assert secs < 2 * timeout_ms / 1000.0                                    # no rank waits beyond the bound
        gat.assert_untouched()
        for l in locs:
            l.assert_unchanged()
        run(torch, solved, world, B, n_costs, root, roll=5)


# ---------------------------------------------------------------------------------------------------------------------
# 9. state and argument errors of a loopback communicator (as for the RCCL one, tests/test_gpu_parity.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors(torch, solved, handles):
    opts = handles[MAX_ITER][:2]
    B, K, M1 = 4, solved.shape[1], MAX_ITER + 1
    loc = Local(torch, solved, 0, B, M1, [1, 2, 3, 4])
    gat = Gathered(torch, 2 * B, K, M1)
    torch.cuda.synchronize()
    group = next(_GROUP)
    L = opts[0].L
    assert opts[0].gather_results_raw(B, loc.sol(), 0, gat.sol()) == api.ERR_STATE          # no communicator yet
    assert L.cilqr_comm_create_loopback(opts[0].h, group, 2, 2, TIMEOUT_MS) == api.ERR_ARG  # a rank outside the world
    assert L.cilqr_comm_create_loopback(opts[0].h, group, 0, 2, 0) == api.ERR_ARG           # no bound
    assert L.cilqr_comm_create_loopback(None, group, 0, 2, TIMEOUT_MS) == api.ERR_NULL
    opts[0].comm_create_loopback(group, 0, 2, TIMEOUT_MS)
    assert L.cilqr_comm_create_loopback(opts[0].h, group, 1, 2, TIMEOUT_MS) == api.ERR_STATE  # one communicator per handle
    assert L.cilqr_comm_create_loopback(opts[1].h, group, 0, 2, TIMEOUT_MS) == api.ERR_ARG    # the rank is taken
    assert L.cilqr_comm_create_loopback(opts[1].h, group, 1, 3, TIMEOUT_MS) == api.ERR_ARG    # another world
    opts[1].comm_create_loopback(group, 1, 2, TIMEOUT_MS)
    # (errors a rank returns before any exchange: one thread will do, nobody waits)
    for o in opts:
        assert o.gather_results_raw(B, loc.sol(), 2, gat.sol()) == api.ERR_ARG              # root outside the world
        assert o.gather_results_raw(B, loc.sol(), -1, gat.sol()) == api.ERR_ARG
        assert o.gather_results_raw(0, loc.sol(), 0, gat.sol()) == api.ERR_ARG
    for o in opts:
        o.comm_destroy()
        assert o.gather_results_raw(B, loc.sol(), 0, gat.sol()) == api.ERR_STATE            # destroyed
        assert L.cilqr_comm_destroy(o.h) == api.ERR_STATE
    torch.cuda.synchronize()
    gat.assert_untouched()
    # the group is gone with its last rank: the same number makes a new one, of another world
    opts[0].comm_create_loopback(group, 0, 1, TIMEOUT_MS)
    opts[0].comm_destroy()
