"""The OSD kernel does not visit the systematic columns of the most reliable basis (kernels/osd.hpp: osd_eliminate).  Its rule,
written out in plain Python (helpers.osd_info_set_novisit), must pick the basis of the reference's plain loop -- on orders with many,
with few and with no steals.  No GPU: test_osd_steals_exact (test_gpu_parity.py) runs the same vectors through the kernel."""
import helpers


def test_osd_novisit_rule_gives_the_plain_basis():
    vectors = helpers.osd_steal_vectors()
    assert len(vectors) == 72
    helpers.osd_steal_checks(vectors)
