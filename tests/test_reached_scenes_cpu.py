"""The constructed scenes of tests/test_gpu_reached_split.py do what they are built for - checked on the CPU oracle's own lists
(the reference's bounding-square lists: a superset of the culled ones, same blend, same n_contrib per pixel up to list position)."""
import torch

import reached_scenes as rs
from test_gpu_raster_parity import forward_state


def test_wall_saturates_in_front_of_the_ball_and_haze_never_saturates(oracle):
    cpu = torch.device("cpu")
    wall, haze = rs.wall(), rs.haze()
    back = torch.arange(rs.P) >= rs.N_SHELL
    for cam in rs.cameras():
        st = forward_state(oracle.backend, wall, cam, cpu, torch.zeros(3), False)
        must, may, listed = rs.list_sets(st, rs.P)
        accepted = st["tiles_touched"] > 0
        # every pixel saturated (the blend stops when T would fall below 1e-4: what is left is below 1e-4 / (1 - 0.9))
        assert float(st["final_T"].max()) < 1e-3
        assert bool(accepted[back].all()) and bool(listed[back].all()) and not bool(may[back].any())
        assert int((accepted & ~must).sum()) >= 0.25 * int(accepted.sum())
        st = forward_state(oracle.backend, haze, cam, cpu, torch.zeros(3), False)
        must, may, listed = rs.list_sets(st, rs.P)
        assert float(st["final_T"].min()) > 0.05 and int(must.sum()) > 1500
