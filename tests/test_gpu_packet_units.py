"""GPU: the packet ray cast of small scenes (csrc/trace.h: packetPass1 + the exact pass) one ray at a time against the oracle's loop over all triangles.  (t, u, v) bit
for bit, prim and the occlusion flag, for EVERY ray of tests/packet_inputs.py -- no exclusions.  The scenes reach what the 12- and 32-triangle scenes of the other tests
do not: one and two triangles, coplanar triangles that are and are not a parallelogram, parallel stacks on each projection axis, 33 and 64 triangles (the 64-bit
candidate mask, bits 32 and 63), a tie in t, coordinates far from the origin.  tests/test_packet_inputs.py holds the census of these inputs."""
import numpy as np
import pytest
from tests import packet_inputs as PI

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", PI.NAMES)
def test_packet_cast_vs_oracle(mi, oracle, name):
    c = PI.case(mi, oracle, name); rays, ref = c["rays"], c["ref"]; gs = mi.Scene(c["sc"])
    got = gs.intersect(rays); occ = gs.intersect(rays, any_hit=True)
    hit = got[:, 3] >= 0
    bad = np.flatnonzero(hit != ref["hit"]); assert len(bad) == 0, (len(bad), bad[:5], rays[bad[:5]])
    h = ref["hit"]
    bad = np.flatnonzero(h)[(bits(got[h, :3]) != bits(ref["tuv"][h])).any(1)]; assert len(bad) == 0, (len(bad), bad[:5], rays[bad[:5]], got[bad[:5]], ref["tuv"][bad[:5]])
    bad = np.flatnonzero(h)[got[h, 3].astype(np.int64) != ref["prim"][h]]; assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5], 3], ref["prim"][bad[:5]])
    bad = np.flatnonzero((occ[:, 3] >= 0) != ref["occ"]); assert len(bad) == 0, (len(bad), bad[:5], rays[bad[:5]])
