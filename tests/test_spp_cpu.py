"""The planner's SPP clause without a device (plan_fusion, host/network.c): both sides of each condition, on edits of spp_unit.cfg."""
import os

import pytest

from yolo_quantization_amd import binding, synth

P5, P9, P13 = "size=5\nstride=1", "size=9\nstride=1", "size=13\nstride=1"


@pytest.mark.parametrize("edits,want", [
    ([], (1, 2, 2)),
    ([("[maxpool]\n" + P13, "[route]\nlayers=-1"), (P5, "size=3\nstride=1"), (P9, "size=5\nstride=1")], (0, 0)),  # 3 / 5 only: below 7
    ([(P9, "size=9\nstride=2"), ("layers=-1,-3,-5,-6", "layers=-1,-5,-6")], (0, 0, 0)),                 # a stride-2 pool between the two others
    ([(P9, "size=8\nstride=1")], (0, 0, 0)),                                                            # an even size
    ([(P9 + "\nquantized=1\nquant_stop=0", P9 + "\nquantized=1\nquant_stop=1")], (0, 0, 0)),            # a float tail on a member
    ([(P5, "size=11\nstride=1"), (P13, "size=5\nstride=1")], (0, 0, 0)),                                # 11 / 9 / 5: out of order
    ([("layers=-2", "layers=-1"), ("layers=-4", "layers=-1")], (0, 0, 0)),                              # a chain: three different inputs
    ([(P13, "size=15\nstride=1")], (0, 0, 0)),                                                          # a 15 beside 5 / 9
    ([("[maxpool]\n" + P13, "[route]\nlayers=-1")], (1, 2)),                                            # two pools 5 / 9
])
def test_planner_clause(cfg_dir, tmp_path, edits, want):
    txt = open(os.path.join(cfg_dir, "spp_unit.cfg")).read()
    for old, new in edits:
        assert txt.count(old) == 1
        txt = txt.replace(old, new)
    cfg, wts = tmp_path / "t.cfg", str(tmp_path / "t.weights")
    cfg.write_text(txt)
    synth.synth_weights(str(cfg), wts, seed=6)
    net = binding.Net(str(cfg), wts, batch=2)
    net.prepare_host_only(1.0 / 255.0, 0)
    pools = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_MAXPOOL]
    assert tuple(net.spp(i) for i in pools) == want
    net.close()
