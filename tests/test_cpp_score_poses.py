"""Scoring a list of poses through the header-only C++ adapter (NdtMatcherHip::scorePosesDev / bestPosesDev /
bestPosesAlignDev and the 3D twins): a small program next to point_fit_smoke.cpp loads a saved map, a scan and a pose
list and calls the three wrappers; the scores, the hits and the refined results must equal the Python matcher's bit for
bit.  Without a GPU the program must compile and fail loudly."""
import os
import subprocess

import numpy as np
import pytest

import point_fit_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SEP = 5, (0.3, 0.05)


@pytest.fixture(scope="module")
def exe(tmp_path_factory, ndt_lib):
    assert hasattr(ndt_lib, "ndt2d_score_poses_dev")
    out = tmp_path_factory.mktemp("cpp") / "score_poses_smoke"
    libdir = os.path.join(ROOT, "gtsam_ndt_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "score_poses_smoke.cpp"), "-o", str(out),
                    "-L", libdir, "-lndt_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"],
                   check=True)
    return str(out)


def _poses(dim, final_pose, m=300):
    rng = np.random.default_rng(2024 + dim)
    p = np.tile(np.asarray(final_pose, dtype=np.float64), (m, 1))
    p[:, :dim] += rng.uniform(-0.6, 0.6, (m, dim))
    p[:, dim:] += rng.uniform(-0.08, 0.08, (m, p.shape[1] - dim))
    p[0] = final_pose
    return p


def _run(exe, tmp_path, dim, blob, scan, poses):
    paths = [str(tmp_path / f"{k}{dim}") for k in ("map", "scan", "poses", "scores")]
    np.ascontiguousarray(blob).tofile(paths[0])
    np.concatenate([np.asarray(c, dtype=np.float32) for c in scan]).tofile(paths[1])
    np.ascontiguousarray(poses, dtype=np.float64).tofile(paths[2])
    return paths, subprocess.run([exe, str(dim), paths[0], paths[1], str(len(scan[0])), paths[2], str(len(poses)), str(K),
                                  repr(SEP[0]), repr(SEP[1]), paths[3]], capture_output=True, text=True, timeout=120)


def test_program_compiles_and_fails_loudly_without_gpu(exe, tmp_path, ndt_lib):
    if ndt_lib.ndt_device_count() > 0:
        return                                      # (covered by the gpu test)
    import map_coarsen_ref as R
    fx = PC.fixture(2)
    blob = R.blob_from_points(np.stack(fx["target"], axis=1), 0.5)[0]
    _, r = _run(exe, tmp_path, 2, blob, fx["source"], _poses(2, fx["final_pose"], 4))
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_scores_hits_and_refinement_through_the_cpp_adapter(exe, tmp_path, gpu_lib, dim):
    import torch
    fx = PC.fixture(dim)
    scan = tuple(np.ascontiguousarray(c[:1500], dtype=np.float32) for c in fx["source"])
    poses = _poses(dim, fx["final_pose"])
    with PC.matcher(dim) as m:
        dev = PC.dev(scan)
        dp = torch.from_numpy(poses).cuda()
        want = m.score_poses(*dev, dp).cpu().numpy()
        hits = m.best_poses(*dev, dp, k=K, min_sep=SEP)
        refined = m.best_poses_align(*dev, dp, k=K, min_sep=SEP)
        paths, r = _run(exe, tmp_path, dim, m.save_map(), scan, poses)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(paths[3], dtype=np.float32).view(np.uint32), want.view(np.uint32))
    assert len(hits) == K and want.max() > 10.0
    rows = [ln.split() for ln in r.stdout.splitlines()]
    num = float.fromhex

    def hit_rows(tag):
        return [(int(w[1]), num(w[2]), tuple(num(v) for v in w[3:])) for w in rows if w[0] == tag]

    expect = [(h.index, h.score, h.pose) for h in hits]
    assert hit_rows("hit") == expect and hit_rows("match") == expect
    got = [(int(w[1]), int(w[2]), int(w[3]), num(w[4]), tuple(num(v) for v in w[5:])) for w in rows if w[0] == "result"]
    assert got == [(q.iterations, q.n_hit, q.status, q.score, q.pose) for _, q in refined]
