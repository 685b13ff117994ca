"""CPU model of the one-launch YZ stage's work distribution (distributedfft_amd/csrc/dfft_zy.hip): tickets, per-plane "published"
counters, prefetch-only-what-is-ready, and the lazy-publish rule "never wait for another workgroup while holding an unpublished
producer unit".  The kernel's two unit loops (eager and lazy) are restated statement by statement as Python generators that yield
wherever another workgroup's action could interleave; a random scheduler (including workgroups that start late, as a grid larger
than the resident set does) drives them.  Checked under many interleavings:
  * the launch terminates (no deadlock), every item is processed exactly once;
  * a consumer unit is loaded only after all producer units of its plane have published;
  * every producer has published when the launch ends (the next execute's done_base arithmetic relies on it);
  * the ticket counter ends at exactly items + 2 * workgroups -- zy_tickets(), what the host adds to its running ticket base.
Negative controls: the lazy loop WITHOUT the flush in front of its blocking wait deadlocks; a loop that prefetches without the
dependency poll loads a consumer unit too early.
Across launches, the host bookkeeping of dfft_fft2d_batch (distributedfft_amd/csrc/dfft_batch.cpp): calls on one cached control block
with changing batch sizes must start every launch with done[p] == done_base on each of its planes; the rule before the fix
(done_base = execs x producers, no reset) breaks that at batch 1 -> 2, and the kernel's range check then raises ZY_ERR_DESYNC.
(Test infrastructure: a model of the protocol, not the kernel's arithmetic --
that is what the -m gpu parity tests are for.)"""
import random

import pytest

NONE, PROD, CONS = 0, 1, 2


class Launch:
    def __init__(self, nplanes, chunk, ua, ub, groups):
        self.nplanes, self.ch, self.ua, self.ub, self.groups = nplanes, chunk, ua, ub, groups
        self.bb = ua + ub
        self.nchunks = (nplanes + chunk - 1) // chunk
        self.total = self.nchunks * chunk * self.bb  # dfft_zy.hip: `total`
        self.ticket = 0
        self.done = [0] * nplanes
        self.processed = {}
        self.violations = []

    def decode(self, t):  # dfft_zy.hip: decode()
        if t >= self.total:
            return (t, NONE, 0, 0)
        c, r = divmod(t, self.ch * self.bb)
        if r < self.ch * self.ua:
            pl = c * self.ch + r // self.ua
            return (t, PROD, pl, r % self.ua) if pl < self.nplanes else (t, NONE, 0, 0)
        r2 = r - self.ch * self.ua
        pl = c * self.ch + r2 // self.ub
        return (t, CONS, pl, r2 % self.ub) if pl < self.nplanes else (t, NONE, 0, 0)

    def is_ready(self, it):
        return it[1] != CONS or self.done[it[2]] >= self.ua

    def load(self, it):
        if it[1] == CONS and self.done[it[2]] < self.ua:
            self.violations.append(("consumer loaded before its plane was published", it))

    def process(self, it):
        key = (it[1], it[2], it[3])
        self.processed[key] = self.processed.get(key, 0) + 1


def workgroup(L, lazy, flush_before_wait=True, poll_before_prefetch=True):
    """One workgroup's life, as a generator; yields ('run',) between steps and ('wait', item) while it spins on a dependency."""
    def take():
        t = L.ticket
        L.ticket += 1
        return t

    def wait_ready(it):
        while not L.is_ready(it):
            yield ("wait", it)

    cur = L.decode(take())
    yield ("run",)
    nxt = L.decode(take())
    yield ("run",)
    if cur[1] != NONE:
        yield from wait_ready(cur)
        L.load(cur)
    pend = None
    nxt_ok = False
    while cur[0] < L.total:
        t2 = take()
        yield ("run",)
        loaded = False
        if nxt[1] != NONE and ((lazy and nxt_ok) or not poll_before_prefetch or L.is_ready(nxt)):
            L.load(nxt)
            loaded = True
        yield ("run",)
        nn_ok = False
        if cur[1] != NONE:
            L.process(cur)  # compute_unit
            yield ("run",)
            if lazy:
                if pend is not None:  # flush(): publish the previous producer unit at the quiet point
                    L.done[pend] += 1
                    pend = None
                nn = L.decode(t2)
                nn_ok = L.is_ready(nn)
                yield ("run",)
                # store_unit
                if cur[1] == PROD:
                    pend = cur[2]
            else:
                # store_unit, then publish at once
                if cur[1] == PROD:
                    L.done[cur[2]] += 1
                nn = L.decode(t2)
        else:
            nn = L.decode(t2)
        yield ("run",)
        if nxt[1] != NONE and not loaded:
            if lazy and flush_before_wait and pend is not None:
                L.done[pend] += 1
                pend = None
            yield from wait_ready(nxt)
            L.load(nxt)
        cur, nxt, nxt_ok = nxt, nn, nn_ok
        yield ("run",)
    if lazy and pend is not None:
        L.done[pend] += 1


def run(L, lazy, seed, late=0, **kw):
    """Drive L.groups workgroups with a random scheduler; `late` of them only start once an earlier one has finished.
    Returns 'ok' or 'deadlock'."""
    rng = random.Random(seed)
    gens = [workgroup(L, lazy, **kw) for _ in range(L.groups)]
    state = ["new"] * L.groups  # new / run / wait / done
    held_back = set(range(L.groups - late, L.groups))
    steps = 0
    while any(s != "done" for s in state):
        steps += 1
        assert steps < 2_000_000, "model did not terminate"
        if any(s == "done" for s in state):
            held_back = set()  # a resident slot became free
        cand = [g for g in range(L.groups) if state[g] != "done" and g not in held_back]
        if not cand:
            held_back = set()
            continue
        # a deadlock: every startable workgroup spins on a dependency nobody left can satisfy
        runnable = [g for g in cand if state[g] != "wait"]
        if not runnable:
            progressed = False
            for g in cand:
                ev = next(gens[g], None)
                if ev is None:
                    state[g], progressed = "done", True
                elif ev[0] != "wait":
                    state[g], progressed = "run", True
            if not progressed and not held_back:
                return "deadlock"
            if not progressed:
                held_back = set()
            continue
        g = rng.choice(cand)
        ev = next(gens[g], None)
        state[g] = "done" if ev is None else ("wait" if ev[0] == "wait" else "run")
    return "ok"


GEOMS = [  # planes, planes per phase, producer units per plane, consumer units per plane, workgroups
    (5, 2, 3, 2, 1), (5, 2, 3, 2, 2), (7, 3, 4, 4, 3), (9, 4, 2, 5, 4), (6, 6, 3, 3, 5), (4, 1, 2, 2, 3), (10, 3, 1, 1, 6),
]


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("geom", GEOMS)
def test_every_interleaving_tried_terminates_and_respects_the_dependencies(geom, lazy):
    nplanes, ch, ua, ub, groups = geom
    for seed in range(60):
        for late in sorted({0, groups // 2, groups - 1}):
            L = Launch(nplanes, ch, ua, ub, groups)
            assert run(L, lazy, seed, late) == "ok", (geom, seed, late)
            assert not L.violations, L.violations[:3]
            want = {(PROD, p, u): 1 for p in range(nplanes) for u in range(ua)}
            want.update({(CONS, p, u): 1 for p in range(nplanes) for u in range(ub)})
            assert L.processed == want
            assert L.done == [ua] * nplanes                 # every producer published by the end of the launch
            assert L.ticket == L.total + 2 * groups         # zy_tickets(): the host's running ticket base


def test_lazy_loop_without_the_flush_before_a_blocking_wait_deadlocks():
    """One workgroup, one plane per phase: after its last producer unit the workgroup's next item is the consumer of that very
    plane -- holding the unit unpublished while waiting for it is a deadlock, and the flush in front of the wait removes it."""
    assert run(Launch(4, 1, 2, 2, 1), True, 0, flush_before_wait=False) == "deadlock"
    assert run(Launch(4, 1, 2, 2, 1), True, 0) == "ok"
    hits = sum(run(Launch(6, 2, 2, 3, 2), True, s, flush_before_wait=False) == "deadlock" for s in range(40))
    assert hits > 0


def test_prefetch_without_the_dependency_poll_is_caught():
    bad = 0
    for seed in range(40):
        L = Launch(7, 3, 4, 4, 3)
        run(L, False, seed, poll_before_prefetch=False)
        bad += bool(L.violations)
    assert bad > 0


# ---- bookkeeping across launches on one cached control block (dfft_fft2d_batch) -----------------------------------------------
M32 = 1 << 32
MAX_PLANES = 64  # (ZY_MAX_PLANES in the library; the rule does not depend on it)


class Ctx:
    """Zy2dCtx and its ZyCtl: done[] per plane, the ticket counter, the host's running ticket base / execute count / last batch."""

    def __init__(self):
        self.done = [0] * MAX_PLANES
        self.ctl_ticket = 0
        self.ticket = self.execs = self.batch = 0


def host_launch(c, batch, ua, tickets, fixed=True):
    """The host side of one call: (ticket_base, done_base) of its launch.  fixed: a batch change zeroes the control block
    (hipMemsetAsync on the caller's stream, ordered after every earlier launch) and restarts the host counters."""
    if fixed and c.batch != batch:
        if c.batch != 0:
            c.done = [0] * MAX_PLANES
            c.ctl_ticket = 0
        c.ticket = c.execs = 0
        c.batch = batch
    base = (c.ticket, (c.execs * ua) % M32)
    c.execs += 1
    c.ticket = (c.ticket + tickets) % M32
    return base


def device_launch(c, batch, ua, tickets):
    """What a launch does to the control block once it has finished: every plane of it gains its ua producer units."""
    for p in range(batch):
        c.done[p] = (c.done[p] + ua) % M32
    c.ctl_ticket = (c.ctl_ticket + tickets) % M32


def guard(done, done_base, need):
    """The kernel's ready() on a plane nothing of this launch has published yet: 'wait', 'ready' or 'desync'."""
    d = (done - done_base) % M32
    return "desync" if d > need else ("ready" if d == need else "wait")


@pytest.mark.parametrize("seed", range(12))
def test_batch_changes_keep_every_plane_in_step_with_done_base(seed):
    rng = random.Random(seed)
    ua = rng.choice([8, 16, 32, 64])
    c = Ctx()
    for _ in range(200):
        batch = rng.choice([1, 2, 3, rng.randint(1, MAX_PLANES)])
        tickets = batch * (ua + rng.randint(1, 64)) + 2 * rng.randint(1, 256)
        ticket_base, done_base = host_launch(c, batch, ua, tickets)
        assert c.ctl_ticket == ticket_base  # the kernel's first-ticket check passes
        for p in range(batch):
            assert c.done[p] == done_base, (p, batch)
            assert guard(c.done[p], done_base, ua) == "wait"  # consumers wait for this launch's producers
        device_launch(c, batch, ua, tickets)
        assert all(guard(c.done[p], done_base, ua) == "ready" for p in range(batch))


def test_old_rule_breaks_at_batch_1_then_2_and_the_guard_catches_it():
    """Negative control: done_base = execs x producers with no reset.  At batch 1 -> 2, plane 1 still counts 0 while done_base is UA:
    the old unsigned test (done - done_base >= need) wraps to 'ready' before any producer has published; the range check raises."""
    ua, tickets = 16, 100
    c = Ctx()
    for batch in (1, 2):
        _, done_base = host_launch(c, batch, ua, tickets, fixed=False)
        if batch == 2:
            assert c.done[0] == done_base
            assert c.done[1] != done_base                               # the invariant is broken ...
            assert (c.done[1] - done_base) % M32 >= ua                  # ... the old test calls plane 1 ready at once ...
            assert guard(c.done[1], done_base, ua) == "desync"          # ... the range check refuses instead
        device_launch(c, batch, ua, tickets)
    # shrink then grow (8 -> 2 -> 8): planes 2..7 lag one execute behind, caught the same way
    c = Ctx()
    for batch in (8, 2, 8):
        _, done_base = host_launch(c, batch, ua, tickets, fixed=False)
        lagging = [p for p in range(batch) if c.done[p] != done_base]
        if lagging:
            assert lagging == list(range(2, 8))
            assert all(guard(c.done[p], done_base, ua) == "desync" for p in lagging)
        device_launch(c, batch, ua, tickets)
    # the fixed rule on the same sequences
    for seq in ((1, 2), (8, 2, 8), (1, 2, 8, 3)):
        c = Ctx()
        for batch in seq:
            _, done_base = host_launch(c, batch, ua, tickets)
            assert c.done[:batch] == [done_base] * batch
            device_launch(c, batch, ua, tickets)
