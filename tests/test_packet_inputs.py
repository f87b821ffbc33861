"""CPU: the inputs of tests/test_gpu_packet_units.py exercise what that test is for.  Every condition is on the INPUTS and the oracle's answers to them -- none on the
code under test: every ray category occurs, more than a quarter of the rays hit, the triangle counts are the ones at which the candidate mask changes width, bits 0, 31,
32 and 63 are closest hits, the tie is a tie, and every quad of a parallel stack is hit by rays that miss its neighbours."""
import numpy as np
import pytest
from tests import packet_inputs as PI


@pytest.mark.parametrize("name", PI.NAMES)
def test_census(mi, oracle, name):
    c = PI.case(mi, oracle, name); sc, rays, cat, ref = c["sc"], c["rays"], c["cat"], c["ref"]; nt = len(sc.idx)
    assert nt == dict(one=1, pgram=2, trapezoid=2, stack_k0=16, stack_k1=16, stack_k2=16, n32=32, n33=33, n64=64, tie=4, far=18)[name] and nt <= 64
    assert 1000 <= len(rays) <= 10000 and np.isfinite(rays[:, :7]).all()
    count = {k: int((cat == i).sum()) for i, k in enumerate(PI.CATS)}
    axis_aligned = name in PI.STACKS + ("tie", "far")
    for k in PI.CATS: assert count[k] > 0 or (k == "parallel_in_plane" and not axis_aligned), (k, count)
    assert ref["hit"].mean() > 0.25, ref["hit"].mean()
    assert np.isinf(rays[:, 7]).mean() > 0.5
    d = rays[:, 4:7]; nz = (d == 0).sum(1)
    assert (nz[cat == PI.CATS.index("one_zero")] == 1).all() and (nz[cat == PI.CATS.index("two_zero")] == 2).all()
    # every triangle index is the closest hit of some ray: with 32 / 33 / 64 triangles that includes bits 0, 31, 32 and 63 of the candidate mask
    closest = set(ref["prim"][ref["hit"]].tolist())
    want = set(range(nt)) - ({1} if name == "tie" else set())
    assert want <= closest, sorted(want - closest)
    for bit in (0, 31, 32, 63):
        if bit < nt: assert bit in closest
    # the interval ends exactly at the hit: with maxt (mint) one float below (above) the hit distance that hit is gone
    for cname, col in (("maxt_at_hit", 7), ("mint_at_hit", 3)):
        sel = cat == PI.CATS.index(cname); assert sel.sum() % 3 == 0 and sel.sum() >= 30
        at = ref["tuv"][sel, 0] == rays[sel, col]; assert at.sum() >= sel.sum() // 4      # the copies with the bound AT the distance still hit there
    if name == "tie":      # triangles 0 and 1 coincide: the oracle names 0 and never 1, and the third coplanar triangle shares many of those hits' planes
        assert 1 not in closest and 0 in closest and 2 in closest
    if name in PI.STACKS:  # rays along the normal through a quad's centre hit that quad (leader missed / follower hit and the reverse: every quad has its turn)
        sel = np.flatnonzero(cat == PI.CATS.index("centroid")); assert len(sel) == 2 * nt
        assert ref["hit"][sel].all() and (ref["prim"][sel] == np.tile(np.arange(nt), 2)).all()
    if name in PI.STACKS + ("far",):      # the rays in a plane: D = 0 and N = 0 for that plane's record
        sel = np.flatnonzero(cat == PI.CATS.index("parallel_in_plane")); assert len(sel) >= 24
    if name == "far":
        assert np.abs(rays[:, :3]).max() > 100 * (sc.pos.max(0) - sc.pos.min(0)).max()
