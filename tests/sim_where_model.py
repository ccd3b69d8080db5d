"""The iteration contract of Model.simulate_where (include/vsrmc.h, csrc/vsr_sim_where.hpp) restated in Python — a helper of test_sim_where_cpu.py /
test_sim_where_gpu.py, not a test.  Nothing here runs the kernel under test: the successors come from Model.get_next_states (k_successors: rows in
(parent, ordinal) order with `err`, pinned against the CPU oracle by the parity tests), the generator is written out below.

In one iteration a walker does exactly one of two things:
  start  it has no walk yet, or its depth equals max_depth, or its state has no enabled instance: it stands on Init.  No draw.
  step   one draw of xorshift64*; pick = draw % (number of enabled instances); the pick-th row in ordinal order is the pair it takes.
All walkers advance one iteration per batched get_next_states call (memoised per record: the small spaces revisit their states)."""
import numpy as np

MASK = (1 << 64) - 1


def splitmix64_stream(seed, n):
    """the first n outputs of splitmix64 started at `seed` — walker i's initial xorshift state is output i, 1 where that is 0"""
    out = []
    x = seed & MASK
    for _ in range(n):
        x = (x + 0x9E3779B97F4A7C15) & MASK
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        out.append(z or 1)
    return out


def xorshift64star(x):
    """-> (next state, draw)"""
    x ^= x >> 12
    x = (x ^ (x << 25)) & MASK
    x ^= x >> 27
    return x, (x * 0x2545F4914F6CDD1D) & MASK


class ErrorRowMet(Exception):
    """an instance that raises an evaluation error is enabled in a visited state: the kernel would end the run there (found = 2)"""


class Walkers:
    """n_walkers walkers over `model` (a vsr_tlaplus_amd.Model).  iterate(n) yields, per iteration, a list with one entry per walker:
    ("start", init_key) or ("step", parent_key, child_key, action id, ordinal), keys being tuples of the wire record's words."""

    def __init__(self, model, n_walkers, max_depth, seed, device=0):
        self.m, self.n, self.max_depth, self.device = model, n_walkers, max_depth, device
        self.rng = splitmix64_stream(seed, n_walkers)
        self.init = tuple(int(x) for x in model.init_state())
        self.cur = [None] * n_walkers
        self.depth = [0] * n_walkers
        self.ords = [[] for _ in range(n_walkers)]
        self.rows = {}                                               # record key -> [(ordinal, action, child key)] of its enabled instances
        self.steps = self.walks = 0

    def _expand(self, keys):
        todo = sorted(set(k for k in keys if k not in self.rows))
        if not todo:
            return
        words = np.array([x for k in todo for x in k], dtype=np.uint64)
        off = np.cumsum([0] + [len(k) for k in todo]).astype(np.uint64)
        out = [[] for _ in todo]
        for s in self.m.get_next_states(words, off, device=self.device, cap_succ=64 * len(todo) + 64):
            if s["err"]:
                raise ErrorRowMet("ordinal %d of a visited state raises error %d" % (s["ordinal"], s["err"]))
            out[s["parent"]].append((s["ordinal"], s["action"], tuple(int(x) for x in s["words"])))
        for k, rows in zip(todo, out):
            assert [r[0] for r in rows] == sorted(r[0] for r in rows)
            self.rows[k] = rows

    def iterate(self, iterations):
        for _ in range(iterations):
            walking = [i for i in range(self.n) if self.cur[i] is not None and self.depth[i] < self.max_depth]
            self._expand(self.cur[i] for i in walking)
            events = []
            for i in range(self.n):
                rows = self.rows[self.cur[i]] if self.cur[i] is not None and self.depth[i] < self.max_depth else []
                if not rows:                                         # start
                    self.cur[i], self.depth[i], self.ords[i] = self.init, 0, []
                    self.walks += 1
                    events.append(("start", self.init))
                    continue
                self.rng[i], draw = xorshift64star(self.rng[i])
                ordinal, action, child = rows[draw % len(rows)]
                events.append(("step", self.cur[i], child, action, ordinal))
                self.cur[i] = child
                self.depth[i] += 1
                self.ords[i].append(ordinal)
                self.steps += 1
            yield events
