"""Run-ahead pacing of the strip MTTKRP kernel (csrc/hip/mttkrp_strip.hip):
a pure-Python model of the slot ring, run under many seeded interleavings.

The protocol: W workgroups make T pace calls each. Call t (0-based) adds 1 to
slot t % S and, for t >= R, waits until slot (t - R) % S has reached
W x ((t - R) // S + 1). A workgroup whose wait times out stops waiting for
good and goes on arriving. The kernel has S = 8 and 0 <= R <= 7; the model
takes any S, so that a ring that is too short (S < R + 1) can be shown to
break the property the ring is there for.

One scheduler step runs one workgroup up to its next shared-memory event: the
add, or one poll of the slot it waits on. Polls that fail leave the workgroup
where it is, so every interleaving of adds and successful polls is
reachable."""
import random

import pytest

S = 8


class Model:
    def __init__(self, W, T, R, slots=S, quitters=()):
        self.W, self.T, self.R, self.S = W, T, R, slots
        self.slot = [0] * slots
        self.arrived = [0] * W          # tickets a workgroup has arrived at
        self.polling = [False] * W      # arrived at its ticket, wait open
        self.waiting = [True] * W
        # quitters give up the first wait they find unmet (a budget of 0)
        self.quitter = [w in quitters for w in range(W)]
        self.timeouts = 0
        self.polled = [0] * W           # waits not met at the first look
        self.spun = [False] * W
        self.early = []                 # (w, ticket) passed before complete
        self.max_lead = 0

    def done(self, w):
        return self.arrived[w] == self.T and not self.polling[w]

    def target_met(self, w):
        u = self.arrived[w] - 1 - self.R
        return self.slot[u % self.S] >= self.W * (u // self.S + 1)

    def runnable(self, w):
        if self.done(w):
            return False
        return not self.polling[w] or self.target_met(w) or self.quitter[w]

    def step(self, w):
        if not self.polling[w]:
            t = self.arrived[w]
            self.slot[t % self.S] += 1
            self.arrived[w] = t + 1
            self.polling[w] = self.waiting[w] and t >= self.R
            self.spun[w] = False
        elif self.target_met(w):
            u = self.arrived[w] - 1 - self.R
            if min(self.arrived) <= u:
                self.early.append((w, u))
            self.polling[w] = False
            self.polled[w] += self.spun[w]
        else:                            # an unmet look of a quitter
            self.spun[w] = True
            self.polled[w] += 1
            self.timeouts += 1
            self.waiting[w] = False
            self.polling[w] = False
        slowest = min(self.arrived)
        for v in range(self.W):
            if self.waiting[v]:
                self.max_lead = max(self.max_lead, self.arrived[v] - slowest)

    def note_blocked(self):
        for w in range(self.W):
            if self.polling[w] and not self.target_met(w):
                self.spun[w] = True

    def run(self, rng):
        """False if the workgroups got stuck (a wait that cannot be met)."""
        while True:
            self.note_blocked()
            ready = [w for w in range(self.W) if self.runnable(w)]
            if not ready:
                return all(self.done(w) for w in range(self.W))
            self.step(rng.choice(ready))


def class_size(T, s, slots=S):
    return len(range(s, T, slots))


@pytest.mark.parametrize("R", range(S))
@pytest.mark.parametrize("W,T", [(2, 5), (3, 17), (5, 40), (8, 9)])
def test_no_wait_ends_early_and_the_lead_is_bounded(W, T, R):
    for seed in range(80):
        m = Model(W, T, R)
        assert m.run(random.Random(1000 * R + seed)), (seed, "stuck")
        # nobody passed its wait on ticket t - R before all W arrived at it
        assert m.early == [], (seed, m.early[:3])
        # a waiting workgroup never leads the slowest by more than R + 1
        assert m.max_lead <= R + 1, (seed, m.max_lead)
        for s in range(S):
            assert m.slot[s] == W * class_size(T, s)
        assert m.timeouts == 0
        assert all(p <= T for p in m.polled)


def test_the_lead_bound_is_reached():
    """R + 1 is tight: one workgroup held back lets another get that far."""
    for R in range(S):
        best = 0
        for seed in range(200):
            m = Model(3, 20, R)
            m.run(random.Random(seed))
            best = max(best, m.max_lead)
        assert best == R + 1, (R, best)


@pytest.mark.parametrize("R", [0, 1, 2, 7])
@pytest.mark.parametrize("quitters", [(0,), (1, 3), (0, 1, 2, 3)])
def test_timed_out_workgroups_keep_the_counts_and_block_nobody(R, quitters):
    W, T = 4, 27
    for seed in range(200):
        m = Model(W, T, R, quitters=quitters)
        # never stuck: what a waiting workgroup waits for always arrives
        assert m.run(random.Random(77 * R + seed)), (seed, "stuck")
        for s in range(S):
            assert m.slot[s] == W * class_size(T, s), (seed, s)
        assert sum(m.arrived) == W * T
        # sticky: at most one time-out per workgroup marked to give up
        assert m.timeouts <= len(quitters)
        # those that kept waiting still never lead by more than R + 1 ...
        assert m.max_lead <= R + 1 or m.timeouts > 0
        assert all(p <= T for p in m.polled)


def test_a_ring_shorter_than_the_run_ahead_plus_one_is_unsound():
    """The model can tell: with S < R + 1 a slot collects arrivals of the
    next lap while a workgroup still waits on the previous one."""
    broken = 0
    for seed in range(200):
        m = Model(3, 12, 2, slots=2)
        m.run(random.Random(seed))
        broken += bool(m.early)
    assert broken > 0
    for seed in range(200):                 # S = R + 1 is enough
        m = Model(3, 12, 2, slots=3)
        assert m.run(random.Random(seed)) and m.early == []
