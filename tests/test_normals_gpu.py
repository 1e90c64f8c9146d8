"""The normal-map kernel on the MI355X (d3d_normals_from_depth; reference mvs/mvs_cas/models/compute_normals.py:32-82) and the
{view}_normal.pfm product of predict_views (--save_normals)."""
import os

import numpy as np
import pytest
import torch

import test_normals as TN
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kernel(depth, K, nei, **kw):
    from deep3d_aerial_amd import ops

    return ops.normals_from_depth(_dev(depth), K, nei=nei, **kw)


@pytest.mark.parametrize("name", TN.FIXTURES)
def test_kernel_against_reference_and_float64(name):
    """Against the float64 evaluation: mean and max chord no worse than twice the reference's own (recorded in the golden
    data).  Against the reference where the summed vector is not near cancellation (|sum| >= 1e-3): within the two errors;
    elsewhere both give a unit vector or both zero.  The border band of width nei is exactly 0."""
    from deep3d_aerial_amd.compute_normals import ComputeNormals

    g = load_golden("normals_" + name)
    for nei in (1, 2):
        if "ref_nei%d" % nei not in g.files:
            continue
        got = ComputeNormals().compute_normal_by_depth(_dev(g["depth"]), torch.from_numpy(g["K"]), nei).cpu().numpy()
        ref = g["ref_nei%d" % nei]
        assert got.shape == ref.shape and got.dtype == np.float32
        f64, norm = TN.normals_f64(g["depth"], g["kinv"], nei)
        ref_mean, ref_max = float(g["ref_chord_mean_nei%d" % nei]), float(g["ref_chord_max_nei%d" % nei])
        mean, mx = TN.chord_stats(got, f64, norm)
        assert mean <= 2.0 * ref_mean and mx <= 2.0 * ref_max, (name, nei, mean, mx, ref_mean, ref_max)
        c = np.linalg.norm(got.astype(np.float64) - ref, axis=-1)[norm >= TN.NORM_FLOOR]
        assert c.size == 0 or c.max() <= 3.0 * ref_max + 1e-7, (name, nei, c.max())
        assert np.array_equal(np.linalg.norm(got, axis=-1) > 0.5, np.linalg.norm(ref, axis=-1) > 0.5)
        B, H, W = g["depth"].shape
        border = np.ones((H, W), bool)
        border[nei:H - nei, nei:W - nei] = False
        assert np.array_equal(got[:, border], np.zeros_like(got[:, border]))
        print("%s nei %d: kernel vs float64 chord mean %.3g max %.3g (reference %.3g / %.3g)" % (name, nei, mean, mx, ref_mean, ref_max))
    if name == "thin":
        assert not _kernel(g["depth"], g["K"], 2).any()   # H == 2 nei


def test_invalid_sizes_raise():
    from deep3d_aerial_amd import ops

    with pytest.raises(RuntimeError, match="smaller than the stencil"):
        ops.normals_from_depth(torch.ones(3, 8, device="cuda"), np.eye(3, dtype=np.float32), nei=2)
    with pytest.raises(ValueError, match="intrinsics"):
        ops.normals_from_depth(torch.ones(2, 8, 8, device="cuda"), np.eye(3, dtype=np.float32))


def _plane_scene(h, w):
    """A noise-free tilted world plane seen by a rotated camera: fp32 depth map, K, and the analytic camera-space normal
    R n_w, oriented towards the camera (negative z)."""
    from deep3d_aerial_amd import synthetic as S

    n_w = np.array([0.12, -0.07, -1.0])
    n_w /= np.linalg.norm(n_w)
    R = S._rot(0.03, -0.02, 0.2)
    C = np.array([15.0, -8.0, 0.0])
    K = np.array([[1.4 * w, 0, (w - 1) / 2.0], [0, 1.4 * w, (h - 1) / 2.0], [0, 0, 1]], np.float64)
    c_w = n_w @ np.array([0.0, 0.0, 600.0])
    ys, xs = np.mgrid[0:h, 0:w]
    rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
    nr = n_w @ R.T
    d = ((c_w - n_w @ C) / (nr @ rays)).reshape(h, w)   # X = C + R^T (d ray): n_w . X = c_w
    n_cam = R @ n_w
    n_cam = n_cam if n_cam[2] < 0 else -n_cam
    return d.astype(np.float32), K.astype(np.float32), n_cam


def test_plane_at_full_size_gives_the_analytic_normal():
    """2752 x 1856 (the map of the fusion tests): mean chord <= 1e-4, max <= 1e-3 against R n_w (fp32 depth rounding alone
    gives 6e-5 / 2.2e-4 in float64)."""
    h, w = 1856, 2752
    d, K, n_cam = _plane_scene(h, w)
    got = _kernel(d, K, 1).cpu().numpy()[1:-1, 1:-1].reshape(-1, 3).astype(np.float64)
    c = np.linalg.norm(got - n_cam, axis=-1)
    print("plane 2752x1856: chord to R n_w mean %.3g max %.3g" % (c.mean(), c.max()))
    assert c.mean() <= 1e-4 and c.max() <= 1e-3


def test_bitwise_determinism_batching_and_path_independence():
    """No atomics: two runs are bit-identical; a batched call equals per-item calls; the 16-byte form (W % 4 == 0, aligned)
    and the scalar form of the kernel give the same bits; the encoded map is (n + 1) / 2 of the same launch."""
    from deep3d_aerial_amd import ops

    h, w = 1856, 2752
    d, K, _ = _plane_scene(h, w)
    rng = np.random.default_rng(3)
    d = d * (1.0 + 0.002 * rng.standard_normal(d.shape)).astype(np.float32)
    dd = _dev(d)
    for nei in (1, 2, 3):
        a = ops.normals_from_depth(dd, K, nei=nei)
        b = ops.normals_from_depth(dd, K, nei=nei)
        assert torch.equal(a, b)
        buf = torch.empty(h * w + 1, dtype=torch.float32, device="cuda")
        shifted = buf[1:].view(h, w)          # contiguous, 4 bytes off 16-byte alignment: the scalar form
        shifted.copy_(dd)
        assert torch.equal(ops.normals_from_depth(shifted, K, nei=nei), a), nei
        n, enc = ops.normals_from_depth(dd, K, nei=nei, encoded=True)
        assert torch.equal(n, a) and torch.equal(enc, (a + 1.0) * 0.5)
        assert torch.equal(ops.normals_from_depth(dd, K, nei=nei, encoded=True, normal=False), enc)
    g = load_golden("normals_batch2")
    for nei in (1, 2):
        both = ops.normals_from_depth(_dev(g["depth"]), g["K"], nei=nei)
        for i in range(2):
            assert torch.equal(both[i], ops.normals_from_depth(_dev(g["depth"][i]), g["K"][i], nei=nei))
    # more items than one launch carries (64): the same bits as per item
    many = _dev(np.repeat(g["depth"][:1], 67, axis=0))
    out = ops.normals_from_depth(many, np.repeat(g["K"][:1], 67, axis=0))
    one = ops.normals_from_depth(_dev(g["depth"][0]), g["K"][0])
    assert all(torch.equal(out[i], one) for i in (0, 63, 64, 66))


def test_compute_normals_forward_layout():
    from deep3d_aerial_amd.compute_normals import ComputeNormals

    g = load_golden("normals_batch2")
    depth = _dev(g["depth"])
    intri = torch.from_numpy(np.stack([g["K"], g["K"][::-1]], 1))     # [B,V,3,3]: view 0 is used
    img = torch.zeros(2, 3, 8, 8, device="cuda")
    out = ComputeNormals()(depth, img, intri)
    assert tuple(out.shape) == (2, 3) + g["depth"].shape[1:]
    want = ComputeNormals().compute_normal_by_depth(depth, torch.from_numpy(g["K"]), 1)
    assert torch.equal(out, want.permute(0, 3, 1, 2))


def _scene_run(tmp_path, tag, **kw):
    import pipeline_scene as PS
    from deep3d_aerial_amd import predict as P

    scene = PS.SceneViews(n=3)
    out = tmp_path / tag
    P.predict_views(PS.SceneModel(scene), scene, str(out), **kw)
    return scene, out


def test_pfm_writer_normal_file_is_save_pfm_of_the_host_copy(tmp_path):
    """--save_normals: {name}_normal.pfm through the asynchronous PfmWriter is byte-identical to save_pfm of the host copy of
    the encoded map, computed with the view's output intrinsics; the other products are unchanged."""
    from deep3d_aerial_amd import ops, predict as P

    scene, out = _scene_run(tmp_path, "on", save_normals=True, normal_nei=2)
    _, plain = _scene_run(tmp_path, "off")
    for i, v in enumerate(scene.views):
        name = "scene_%02d" % i
        enc = ops.normals_from_depth(_dev(v["depth"]), scene[i]["outcam"][1, :3, :3], nei=2, encoded=True, normal=False)
        P.save_pfm(str(tmp_path / "want.pfm"), enc.cpu().numpy())
        assert (out / ("%s_normal.pfm" % name)).read_bytes() == (tmp_path / "want.pfm").read_bytes(), name
        n, _ = P.load_pfm(str(out / ("%s_normal.pfm" % name)))
        assert np.abs((n * 2.0 - 1.0) - ops.normals_from_depth(_dev(v["depth"]), v["K"], nei=2).cpu().numpy()).max() <= 1.2e-7
        for suffix in ("_init.pfm", "_prob.pfm", ".txt"):
            assert (out / (name + suffix)).read_bytes() == (plain / (name + suffix)).read_bytes()


def test_predict_views_without_the_flag_writes_what_it_wrote_before(tmp_path):
    _, out = _scene_run(tmp_path, "off")
    names = ["scene_%02d" % i for i in range(3)]
    assert sorted(os.listdir(out)) == sorted(n + s for n in names for s in ("_init.pfm", "_prob.pfm", ".txt"))
