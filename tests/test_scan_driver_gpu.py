"""The one statement that spans every consumer of the slice driver (csrc/host_step_slices.hpp; `-m gpu`): on BASELINE config 1 (R=2, C=1, n=1, L=1: 76
states, 14 levels), level by level, the transitions out of the level counted three ways — the pairs of a TRUE step scan (step_run), `pairs` of an action
constraint TRUE (phase_expand_gated) and `generated` of the plain checker (k_expand) — are one number, the CPU oracle's, whether a slice holds one parent,
three, or the whole level."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = dict(table_log2=16, frontier_words=1 << 18, frontier_states=1 << 14, pending_entries=1 << 15)
KNOBS = ("VSRMC_STEP_SLICE", "VSRMC_ACTION_SLICE")


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.fixture(scope="module")
def oracle_generated():
    """generated[k] = the successors of level k + 1, from the oracle: computed once, shared, never changed"""
    from oracle import orc
    ob = orc.Bfs(orc.Params(2, 1, 1, 1))
    out = []
    while True:
        nn = ob.step()
        out.append((ob.info["generated"], nn))
        if nn == 0:
            return out


@pytest.mark.parametrize("slice_", [1, 3, None])
def test_three_counts_of_a_level_agree(vt, oracle_generated, monkeypatch, slice_):
    assert len(oracle_generated) == 14 and sum(nn for _g, nn in oracle_generated) == 75
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
        if slice_ is not None:
            monkeypatch.setenv(k, str(slice_))
    m = vt.Model.from_constants(R=2, C_=1, n=1, L=1)
    w = m.compile_step_predicates("True == TRUE")
    plain = vt.ModelChecker(m, device=0, **SIZES)
    gated = vt.ModelChecker(m, device=0, **SIZES)
    gated.action_constrain(w)
    for level, (generated, n_new) in enumerate(oracle_generated, start=1):
        parents, parents_g = plain.n_frontier, gated.n_frontier
        t = plain.step_scan(w)
        d = plain.step()
        dg = gated.step()
        ai = gated.action_constraint_results(0)
        print("level %d: step scan %d pairs in %d listings, action constraint %d pairs in %d, k_expand %d, oracle %d"
              % (level, t["n_pairs"], t["slices"], ai["pairs"], ai["slices"], d["generated"], generated))
        assert t["n_err"] == 0 and ai["blocked"] == 0
        assert t["n_pairs"] == ai["pairs"] == d["generated"] == dg["generated"] == generated, level
        assert d["n_new"] == dg["n_new"] == n_new, level
        if slice_ is not None:                                       # the knob reached both loops: a listing per slice_ parents, none void
            assert t["slices"] >= (parents + slice_ - 1) // slice_, level      # (k_expand's level is an index range with withdrawn indices: at least its states)
            assert ai["slices"] == (parents_g + slice_ - 1) // slice_ and ai["relisted"] == 0, level   # (the gated level is dense)
    assert plain.distinct == gated.distinct == 76
    plain.close()
    gated.close()
