"""The iteration contract of Model.simulate_constrained (include/vsrmc.h, csrc/vsr_sim_constrain.hpp) restated in Python — a helper of
test_sim_constrained_gpu.py, not a test.  It extends sim_where_model.Walkers (the generator, the memoised successor rows of Model.get_next_states) with the
tried set and the four outcomes.  Nothing here runs the kernel under test; the verdicts are the caller's Python functions (constraint_reference.py,
action_constraint_reference.py and the predicate references), never a compiled program.

In one iteration a walker does exactly one of four things:
  start    no walk yet, or depth == max_depth, or no enabled instance, or every enabled instance tried (`stuck` + 1): it stands on Init, tried set cleared.
           No draw.
  blocked  one draw; pick = draw % (untried instances), over the untried rows in ordinal order; step_ok(parent, child, action) is false: the position is
           marked tried, the walker stays.
  pruned   ... step_ok holds (or there is no action constraint) and state_ok(child) is false: the position is marked tried, the walker stays.
  step     both hold: the walker moves, tried set cleared."""
import sim_where_model as sm

TRIED_BITS = 256


class ConstrainedWalkers(sm.Walkers):
    """iterate(n) yields, per iteration, one entry per walker: ("start", init_key) or (kind, parent_key, child_key, action id, ordinal) with kind in
    "blocked", "pruned", "step".  state_ok(child_key) / step_ok(parent_key, child_key, action id): the constraints, None = not attached."""

    def __init__(self, model, n_walkers, max_depth, seed, state_ok=None, step_ok=None, device=0):
        sm.Walkers.__init__(self, model, n_walkers, max_depth, seed, device)
        self.state_ok, self.step_ok = state_ok, step_ok
        self.tried = [set() for _ in range(n_walkers)]
        self.blocked = self.pruned = self.stuck = 0
        self.max_enabled = 0                                         # the largest number of enabled instances of a state a walker tried to leave

    def iterate(self, iterations):
        for _ in range(iterations):
            walking = [i for i in range(self.n) if self.cur[i] is not None and self.depth[i] < self.max_depth]
            self._expand(self.cur[i] for i in walking)
            events = []
            for i in range(self.n):
                rows = self.rows[self.cur[i]] if self.cur[i] is not None and self.depth[i] < self.max_depth else []
                assert len(rows) <= TRIED_BITS, "the kernel would end the run here: VSRMC_SIM_ERR_TRIED_WIDTH"
                if not rows or len(self.tried[i]) >= len(rows):      # start
                    self.stuck += bool(rows)
                    self.cur[i], self.depth[i], self.ords[i], self.tried[i] = self.init, 0, [], set()
                    self.walks += 1
                    events.append(("start", self.init))
                    continue
                self.max_enabled = max(self.max_enabled, len(rows))
                self.rng[i], draw = sm.xorshift64star(self.rng[i])
                untried = [p for p in range(len(rows)) if p not in self.tried[i]]
                pos = untried[draw % len(untried)]
                ordinal, action, child = rows[pos]
                ev = (self.cur[i], child, action, ordinal)
                if self.step_ok is not None and not self.step_ok(self.cur[i], child, action):
                    self.tried[i].add(pos)
                    self.blocked += 1
                    events.append(("blocked",) + ev)
                elif self.state_ok is not None and not self.state_ok(child):
                    self.tried[i].add(pos)
                    self.pruned += 1
                    events.append(("pruned",) + ev)
                else:
                    self.cur[i] = child
                    self.depth[i] += 1
                    self.ords[i].append(ordinal)
                    self.tried[i] = set()
                    self.steps += 1
                    events.append(("step",) + ev)
            yield events


def model_counts(action_names, m, unpack, n_walkers, max_depth, seed, iterations, state_preds=(), state_bits=None, state_con=None, step_preds=(),
                 step_bits=None, step_con=None):
    """The figures the contract gives for `iterations` iterations.  state_preds / step_preds: the exported predicates (name, text, python function) in
    program order, evaluated by state_bits(preds, view) / step_bits(preds, parent view, child view, action name); state_con / step_con: the index of the
    constraint among them (None: not attached).  The bits of a state are counted when a walker stands on it (start, step), the bits of a pair when the
    step is taken — a blocked or pruned try counts nothing but itself."""
    views, sb, pb = {}, {}, {}

    def view(key):
        if key not in views:
            views[key] = unpack(list(key))
        return views[key]

    def s_bits(key):
        if key not in sb:
            sb[key] = state_bits(state_preds, view(key))
        return sb[key]

    def p_bits(parent, child, action):
        if (parent, child, action) not in pb:
            pb[(parent, child, action)] = step_bits(step_preds, view(parent), view(child), action_names[action])
        return pb[(parent, child, action)]

    W = ConstrainedWalkers(m, n_walkers, max_depth, seed,
                           state_ok=None if state_con is None else (lambda key: bool((s_bits(key) >> state_con) & 1)),
                           step_ok=None if step_con is None else (lambda p, c, a: bool((p_bits(p, c, a) >> step_con) & 1)))
    cs, cp = [0] * len(state_preds), [0] * len(step_preds)
    n_states = n_pairs = 0
    for events in W.iterate(iterations):
        for ev in events:
            if ev[0] in ("blocked", "pruned"):
                continue
            if state_preds:
                bits = s_bits(ev[1] if ev[0] == "start" else ev[2])
                n_states += 1
                for k in range(len(state_preds)):
                    cs[k] += (bits >> k) & 1
            if ev[0] == "step" and step_preds:
                bits = p_bits(ev[1], ev[2], ev[3])
                n_pairs += 1
                for k in range(len(step_preds)):
                    cp[k] += (bits >> k) & 1
    return dict(cs=cs, cp=cp, n_states=n_states, n_pairs=n_pairs, steps=W.steps, walks=W.walks, blocked=W.blocked, pruned=W.pruned, stuck=W.stuck,
                max_enabled=W.max_enabled, walkers=W)
