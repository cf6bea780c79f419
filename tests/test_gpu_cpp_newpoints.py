"""USLAM::ORBmatcher::CreateNewMapPoints (include/uvo/compat/ORBmatcher.h) driven from a C++ program through the C ABI, the way
LocalMapping::CreateNewMapPoints would drive it; checked against the Python binding of the same entry point and, on the scene without
sensitive matches, against the loop it replaces (SearchForTriangulationBegin / Next + the triangulation on the host)."""
import json
import os
import subprocess

import numpy as np
import pytest

import host_build
import triangulation_model as tm

def build_driver():
    return host_build.build("compat_newpoints")


def test_new_points_driver_compiles_as_cxx11(uvo):
    """The new adaptor member instantiates with stand-in key frame types in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [False, True])
@pytest.mark.parametrize("name", ["twenty_pairs", "twenty_pairs_b"])
def test_cpp_create_new_map_points(uvo, tmp_path, name, ori):
    driver = build_driver()
    sc = tm.make_scene(**tm.SCENES[name])
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    tm.write_scene_file(scene_p, sc, ori)
    r = subprocess.run([driver, scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    one, host = tm.read_new_points_file(out_p, len(sc["pairs"]))
    # the same entry point through the Python binding: same library, same inputs, so the same bits
    m = uvo.ORBmatcher(0.6, ori)
    pairs = [(uvo.FeatureVector(P["groups"]), P["kp"], P["desc"], P["has_mp"], P["F12"], P["sigma2"]) for P in sc["pairs"]]
    cam = lambda c: uvo.TriangulationCamera(c.rcw, c.tcw, c.ow, c.fx, c.fy, c.cx, c.cy, c.sf, c.sigma2)
    dev, _ = m.CreateNewMapPoints(uvo.FeatureVector(sc["groups1"]), sc["kp1"], sc["desc1"], sc["has_mp1"], pairs, cam(sc["cam1"]),
                                  [cam(c) for c in sc["cams2"]], sc["ratio_factor"])
    m.close()
    total = 0
    for k, (d, (i1, i2, x)) in enumerate(zip(dev, one)):
        ok = d["verdict"] == tm.ACCEPTED
        np.testing.assert_array_equal(i1, d["idx1"][ok], err_msg="pair %d" % k)
        np.testing.assert_array_equal(i2, d["idx2"][ok], err_msg="pair %d" % k)
        np.testing.assert_array_equal(x, d["x3d"][ok], err_msg="pair %d" % k)
        total += len(i1)
    assert total == info["new_points_one_call"] and total > 150
    if name == tm.SCENE_WITHOUT_SENSITIVE:
        # no match of this scene sits near a threshold: the loop the call replaces (host triangulation between the pairs) accepts the same
        # matches, and its points agree within the kernel's bound against each other's common float64 truth (2 x X3D_BOUND apart at most)
        for k, ((i1, i2, x), (h1, h2, hx)) in enumerate(zip(one, host)):
            np.testing.assert_array_equal(i1, h1, err_msg="pair %d: host loop" % k)
            np.testing.assert_array_equal(i2, h2, err_msg="pair %d: host loop" % k)
            if len(x):
                assert tm.rel_dev(hx, x.astype(np.float64)).max() <= 2 * tm.X3D_BOUND
