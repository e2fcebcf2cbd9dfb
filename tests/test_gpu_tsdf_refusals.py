"""Which check wins, and what it says, for every public call of the TSDF family whose host driver is shared between variants
(tests/tsdf_refusals_fixture.py): in each of five contexts -- no volume, dense, dense + colour, hashed, hashed + colour -- every call of the
fixture's TABLE with valid arguments and with every bad argument that applies, the status and the whole icp_last_error string against
tests/golden/tsdf_refusals.json, entry by entry.  The golden file was recorded from a library built from commit 9cecfae, before the
per-variant host code was folded: a fold that reorders two checks changes which message a state gets, and fails here."""
import json
import pytest

import tsdf_refusals_fixture as RF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(RF.GOLDEN) as f:
        g = json.load(f)
    assert g["produced_by"] == RF.PRODUCED_BY
    return g["contexts"]


@pytest.mark.parametrize("name", RF.CONTEXTS)
def test_every_call_answers_as_before(gpu_ctx_factory, golden, name):
    want = golden[name]
    assert list(want) == RF.keys()                         # every entry of the table is in the file, none left out
    got = RF.record(RF.make_context(gpu_ctx_factory, name))
    assert list(got) == RF.keys()
    wrong = []
    for key in RF.keys():
        if key.endswith("/valid") and want[key]["status"] == 0:
            if got[key]["status"] != 0:                    # valid arguments in a state that takes the call: status 0 only
                wrong.append((key, got[key], want[key]))
        elif got[key] != want[key]:
            wrong.append((key, got[key], want[key]))
    assert not wrong, "%s: %d of %d entries differ (key, got, recorded): %s" % (name, len(wrong), len(want), wrong[:6])


def test_valid_calls_succeed_where_the_state_takes_them(golden):
    """The fixture's shapes do find a surface: in the state a call is made for, its valid-argument entry was recorded with status 0."""
    home = {"icp_tsdf_raycast": "dense", "icp_tsdf_raycast_color": "dense_color", "icp_tsdf_raycast_hashed": "hashed", "icp_tsdf_raycast_color_hashed": "hashed_color",
            "icp_set_target_tsdf": "dense", "icp_set_target_tsdf_color": "dense_color", "icp_set_target_tsdf_hashed": "hashed", "icp_set_target_tsdf_color_hashed": "hashed_color",
            "icp_tsdf_mesh": "dense", "icp_tsdf_mesh_color": "dense_color", "icp_tsdf_mesh_hashed": "hashed", "icp_tsdf_mesh_color_hashed": "hashed_color"}
    for fn, _, _ in RF.TABLE:
        for name in ([home[fn]] if fn in home else ["dense_color", "hashed_color"]):
            assert golden[name][fn + "/valid"] == dict(status=0, error=""), (name, fn, golden[name][fn + "/valid"])
