"""The realtime tracking plans launch for launch against tests/golden/track_plans.json (tests/track_plan_fingerprint.py): the golden
file was written at the commit before hipdp.ops' plain / _ix / _src wrapper triplets became one op per launch, so equality here says
that every plan still names the same C symbols in the same order with the same argument values -- the device does what it did."""
import json

import pytest

from tests import track_plan_fingerprint as F
from tests.backends import BACKENDS, get_runtime


@pytest.mark.parametrize('backend', BACKENDS)
def test_track_plans_are_the_pinned_launches(backend):
    want = F.load_golden()[backend]
    got = json.loads(json.dumps(F.fingerprints(get_runtime(backend), backend)))
    assert sorted(got) == sorted(want)
    assert len(want) == 8 + 16 + 8 + 1                                  # HandTracker, MultiTracker, the detectors, refine_stage
    for case in sorted(want):
        assert len(got[case]) == len(want[case]), case
        for i, (g, w) in enumerate(zip(got[case], want[case])):
            assert g == w, (case, i)
    # the families are all there: a fingerprint that pinned one family three times would pass the equality above as well
    symbols = set(row[1] for rows in want.values() for row in rows)
    for stem in ('crop_prepare_ranged', 'crop_warp', 'track_refine', 'crop_warp_ex', 'pose_finish'):
        assert set('dpp_' + stem + s for s in ('', '_ix', '_src')) <= symbols, stem
    for stem in ('frame_range', 'frame_ingest'):
        assert set('dpp_' + stem + s for s in ('', '_src')) <= symbols, stem
    assert set(['dpp_pose_fuse', 'dpp_refine_com_iterative', 'dpp_refine_com_iterative_ix']) <= symbols
