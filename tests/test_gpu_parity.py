"""Parity tests proper (need an MI355X): the HIP path, called through the C-ABI, against the CPU oracle on the same
seeded inputs, against the committed golden fixtures, and -- at BASELINE.json's full sizes, where the oracle would
take hours -- through size-independent properties (BVH walk == linear scan, row-range / sharding / launch-geometry
invariance, determinism).

Tolerance: north_star asks for image RMSE < 1e-4 on the linear float framebuffer.  The HIP path keeps the reference's
fp32 operation order (no FMA contraction, IEEE sqrt/div), so the bar used here is stricter: BIT-EXACT floats, except
that powf(x, 5) in the Schlick term is evaluated through double on the GPU and by libm on the CPU; a 1-ulp difference
there flips a sample only when a 32-bit uniform lands in the 1-ulp gap (~1e-8 per dielectric hit), so a handful of
differing pixels per full frame is tolerated via `_assert_frames_equal(max_pixels=...)` and RMSE is always checked."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.scenes import arrays, big_grid, cornell_like, random_spheres, three_spheres, three_spheres_camera

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4  # north_star: image RMSE < 1e-4 vs the CPU path on the same seeded scene


def _assert_frames_equal(got, want, max_pixels=0):
    assert got.shape == want.shape
    if got.size == 0:
        return
    # a NaN is a NaN: the reference arithmetic can produce one (glm::refract returns the zero vector when rounding
    # makes k < 0 although eta * sin <= 1 held; the next ray has a zero direction and its sky colour is 0 * inf), and
    # the payload bits of a NaN differ between x86 and gfx950.  RGBAColor maps it to black on both sides.
    both_nan = np.isnan(got) & np.isnan(want)
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~both_nan
    if diff.ndim == 3:
        diff = diff.any(axis=-1)
    delta = np.where(both_nan, 0.0, got.astype(np.float64) - want.astype(np.float64))
    rmse = float(np.sqrt(np.mean(delta ** 2)))
    assert rmse < RMSE_TOL, rmse
    assert int(diff.sum()) <= max_pixels, f"{int(diff.sum())} pixels differ (rmse {rmse:.3e})"


def _both(pkg):
    return ((pkg.ACCEL_BVH, "bvh"), (pkg.ACCEL_BRUTE, "brute"))


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("marked gpu but no GPU is visible: the product has no CPU fallback")
    return torch


# ---------------------------------------------------------------------------------------------------------------
# golden fixtures and oracle parity at oracle-sized problems
# ---------------------------------------------------------------------------------------------------------------
def test_golden_rtow_counter_frame(pkg, gpu):
    g = np.load(os.path.join(GOLDEN, "rtow_counter_128x72x16.npz"))
    sc = np.load(os.path.join(GOLDEN, "rtow_scene_seed12345.npz"))
    cp = json.loads(str(g["camera"]))
    cam = pkg.camera_setup(pkg.camera_params(**cp))
    for accel, _ in _both(pkg):
        with pkg.Scene(cam, sc["objects"], sc["materials"], accel=accel) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, int(g["seed"]))
        _assert_frames_equal(rgb, g["rgb"])
        assert np.array_equal(rgba, g["rgba"])


def test_golden_cornell_deep_bounce(pkg, gpu):
    """config 5 shape: enclosed box, 200 bounces."""
    g = np.load(os.path.join(GOLDEN, "cornell_counter_48x48x32.npz"))
    cp = json.loads(str(g["camera"]))
    cam = pkg.camera_setup(pkg.camera_params(**cp))
    for accel, _ in _both(pkg):
        with pkg.Scene(cam, g["objects"], g["materials"], accel=accel) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, int(g["seed"]))
        _assert_frames_equal(rgb, g["rgb"])
        assert np.array_equal(rgba, g["rgba"])


def test_config1_three_lambertian_spheres(pkg, ob, gpu):
    """BASELINE config 1: 3-sphere Lambertian scene, 400x225, 1 spp, 1 bounce."""
    objs, mats = three_spheres()
    kw = three_spheres_camera()
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    assert (cam.img_width, cam.img_height) == (400, 225)
    want, want8 = ob.render_rect_counter(ocam, objs, mats, 1, 0, 0, 400, 225, nthreads=8)
    for accel, _ in _both(pkg) + ((pkg.ACCEL_AUTO, "auto"),):
        with pkg.Scene(cam, objs, mats, accel=accel) as s:
            rgb, rgba = s.render_rows(0, 225, 1)
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)


@pytest.mark.parametrize("width,spp,depth,seed", [(160, 8, 50, 1), (96, 32, 50, 0xDEADBEEFCAFE), (101, 3, 7, 9),
                                                  (64, 1, 1, 3), (64, 2, 0, 3), (48, 64, 3, 2 ** 63 + 5)])
def test_rtow_matches_oracle(pkg, ob, rtow, gpu, width, spp, depth, seed):
    kw = dict(image_width=width, samples_per_pixel=spp, max_depth=depth)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, want8 = ob.render_rect_counter(ocam, *rtow, seed, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
    for accel, _ in _both(pkg):
        with pkg.Scene(cam, *rtow, accel=accel) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, seed)
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)


def test_no_defocus_and_other_cameras(pkg, ob, rtow, gpu):
    for kw in (dict(image_width=80, samples_per_pixel=4, max_depth=20, defocus_angle=0.0),
               dict(image_width=72, samples_per_pixel=4, max_depth=20, defocus_angle=10.0, focus_distance=3.4,
                    lookfrom=(-2.0, 2.0, 1.0), lookat=(0.0, 0.0, -1.0), vertical_fov=90.0),
               dict(image_width=50, aspect_ratio=1.7, samples_per_pixel=8, max_depth=8)):
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        want, _ = ob.render_rect_counter(ocam, *rtow, 4, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
        with pkg.Scene(cam, *rtow) as s:
            rgb, _ = s.render_rows(0, cam.img_height, 4)
        _assert_frames_equal(rgb, want)


def test_random_spheres_mixed_radii(pkg, ob, gpu):
    """BVH stress: 3000 spheres of mixed radii; BVH walk, linear scan and oracle agree."""
    objs, mats = random_spheres(3000, seed=5)
    kw = dict(image_width=64, samples_per_pixel=4, max_depth=30, lookfrom=(16.0, 3.0, 5.0))
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, _ = ob.render_rect_counter(ocam, objs, mats, 8, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
    for accel, _ in _both(pkg):
        with pkg.Scene(cam, objs, mats, accel=accel) as s:
            rgb, _ = s.render_rows(0, cam.img_height, 8)
        _assert_frames_equal(rgb, want)


def test_hbm_resident_scene_variant(pkg, ob, rtow, gpu):
    """Scenes that do not fit LDS are traversed out of HBM (config 4 path); forced here on the RTOW scene so that the
    same frame is checked through both memory layouts."""
    kw = dict(image_width=96, samples_per_pixel=8, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, want8 = ob.render_rect_counter(ocam, *rtow, 12, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
    for accel, _ in _both(pkg):
        with pkg.Scene(cam, *rtow, accel=accel, tuning=dict(force_hbm_scene=1)) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, 12)
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)


def test_launch_info_reports_what_the_tuning_resolved_to(pkg, rtow, gpu):
    """rtmi_scene_get_launch_info: the RTOW scene is staged into LDS with two 768-lane workgroups per CU (6 waves per
    SIMD); forcing the HBM layout, another block size or the queue-scheduled kernel shows up in the report."""
    cam = pkg.camera_setup(pkg.camera_params(image_width=64, samples_per_pixel=2, max_depth=8))
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH) as s:
        li = s.launch_info()
    assert li["kernel"] == 1 and li["block_lanes"] == 768 and li["blocks_per_cu"] == 2 and li["scene_in_lds"] == 1
    assert li["grid_blocks"] % 2 == 0 and 0 < li["lds_bytes"] <= 80 * 1024 and li["stack_depth"] >= 3
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, tuning=dict(force_hbm_scene=1, block_lanes=512)) as s:
        li2 = s.launch_info()
    assert li2["scene_in_lds"] == 0 and li2["block_lanes"] == 512 and li2["lds_bytes"] < li["lds_bytes"]
    # the queue-scheduled kernel of round 2 (slower on every workload) was removed in round 4: asking for it fails loudly
    # instead of silently running something else
    with pytest.raises(pkg.RtmiError) as e:
        pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, tuning=dict(kernel=2))
    assert e.value.code == pkg.RTMI_ERR_UNSUPPORTED
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, tuning=dict(blocks_per_cu=1)) as s:
        assert s.launch_info()["blocks_per_cu"] == 1
        # a caller built against the 40-byte rtmi_launch_info of version 0.3 gets the fields it knows and nothing beyond them
        import ctypes as C
        old = (C.c_uint32 * 13)(*([40] + [0xdeadbeef] * 12))
        assert pkg.lib().rtmi_scene_get_launch_info(s._h, C.cast(old, C.POINTER(pkg.LaunchInfo))) == 0
        assert old[1] == 1 and old[4] == 1 and list(old[10:]) == [0xdeadbeef] * 3
        old[0] = 36
        assert pkg.lib().rtmi_scene_get_launch_info(s._h, C.cast(old, C.POINTER(pkg.LaunchInfo))) == pkg.RTMI_ERR_BAD_ARG
    # HBM-resident trees: the top of the tree is staged into LDS (as many breadth-first nodes as fit next to the stacks; here the
    # whole 288-node tree, and with walk starts the 4 + 16 + 64 + 256 slots of the top way records, placed by path code),
    # rtmi_tuning::lds_top_nodes caps it (n > 0: at most n - 1 records)
    for cap, want_top in ((0, None), (1, 0), (41, 40)):
        with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, tuning=dict(force_hbm_scene=1, lds_top_nodes=cap)) as s:
            li3 = s.launch_info()
            assert li3["scene_in_lds"] == 0 and li3["lds_top_nodes"] == (s.bvh()["n_tree_nodes"] + 340 if want_top is None else want_top)  # (the whole tree + the block of top way records)
            assert li3["pad_mode"] == 1
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BRUTE) as s:
        assert s.launch_info()["pad_mode"] == 0 and s.launch_info()["lds_top_nodes"] == 0


def test_scheduling_knobs_do_not_change_the_image(pkg, ob, rtow, gpu):
    """Sample-chunk work items, launch geometry and the traversal exit threshold are scheduling decisions: every
    combination yields the oracle's frame bit for bit."""
    kw = dict(image_width=128, samples_per_pixel=96, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, want8 = ob.render_rect_counter(ocam, *rtow, 44, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
    for env in (dict(chunk_samples=-1), dict(chunk_samples=16), dict(chunk_samples=3, block_lanes=640),
                dict(chunk_samples=32, sample_buf_mb=1), dict(chunk_samples=40, block_lanes=256, wait_thresh=20),
                dict(blocks_per_cu=1, wait_thresh=64, top_down=1)):
        with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, collect_stats=True, tuning=env) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, 44)
            st = s.stats()
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)
        assert st["samples"] == cam.img_width * cam.img_height * 96, env


def test_packed_and_run_length_attenuation_chains(pkg, ob, rtow, gpu):
    """The attenuation chain of a path (core.cc:247-248 multiplies innermost-first) has two forms: packed material handles
    in LDS that leave with the sample record and are multiplied by the resolve pass (scenes whose strings fit: the box of
    config 5, anything with a low bounce limit), and run-length encoded runs multiplied at path end (RTOW at 50 bounces).
    Both give the oracle's frame bit for bit: whole calls, banded calls, sharded row blocks, whole-pixel work items."""
    torch = gpu
    g = np.load(os.path.join(GOLDEN, "cornell_counter_48x48x32.npz"))
    ccam = pkg.camera_setup(pkg.camera_params(**json.loads(str(g["camera"]))))
    for tun, packed in ((None, True), (dict(chain_mode=1), False), (dict(sample_buf_mb=1), True), (dict(chunk_samples=-1), True),
                        (dict(block_lanes=512, chunk_samples=5), True), (dict(gen_ahead=1, chunk_samples=3), True),
                        (dict(chunk_samples=2), True)):
        for accel, _ in _both(pkg):
            with pkg.Scene(ccam, g["objects"], g["materials"], accel=accel, tuning=tun) as s:
                assert (s.launch_info()["packed_chains"] > 0) == packed
                assert s.launch_info()["gen_ahead"] == 0  # (round 5's primary rays generated ahead are out again; the knob is ignored)
                rgb, rgba = s.render_rows(0, ccam.img_height, int(g["seed"]))
                part, _ = s.render_rows(7, 19, int(g["seed"]))
                assert s.launch_info()["packed_chain_fallbacks"] == 0  # what was launched is what the scene is eligible for
            _assert_frames_equal(rgb, g["rgb"])
            assert np.array_equal(rgba, g["rgba"])
            _assert_frames_equal(part, g["rgb"][7:19])
    # RTOW: 488 materials = 9 bits a bounce; packed at 12 bounces, run-length encoded at 50
    for depth, packed in ((12, True), (50, False)):
        kw = dict(image_width=112, samples_per_pixel=10, max_depth=depth)
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        want, want8 = ob.render_rect_counter(ocam, *rtow, 8, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
        for tun in (None, dict(chain_mode=1)):
            with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, tuning=tun) as s:
                assert (s.launch_info()["packed_chains"] > 0) == (packed and tun is None)
                rgb, rgba = s.render_rows(0, cam.img_height, 8)
                # sharded row blocks through the device-pointer entry (three ranks' worth on one device)
                dev = torch.device("cuda", 0)
                plan = pkg.RowShardPlan(cam.img_height, 8, 3)
                parts = []
                for r in range(3):
                    y_first, n_blocks, rows = plan.shard(r)
                    buf = torch.zeros((plan.max_rows, cam.img_width, 3), dtype=torch.float32, device=dev)
                    s.render_row_blocks_device(y_first, 8, 3, n_blocks, 8, buf.data_ptr(), 0, torch.cuda.current_stream(dev).cuda_stream)
                    torch.cuda.synchronize()
                    parts.append(buf)
                frame = torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev)).cpu().numpy()
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8)
            _assert_frames_equal(frame, want)


def test_packed_chain_word_geometry(pkg, ob, gpu):
    """The packed chain's geometry follows the material count and the bounce limit: 1 bit a handle (32 to a word) for one or
    two materials up to 9 bits (3 to a word), slots of 4 to 16 words, chains that end exactly at a word boundary or one
    handle past it -- every combination against the oracle, with the packed form actually in use."""
    rng = np.random.default_rng(11)
    for n_mats, depth in ((1, 33), (2, 64), (3, 16), (4, 17), (5, 10), (8, 11), (9, 8), (17, 7), (33, 30), (100, 50), (300, 40)):
        n = 12  # (fewer spheres than materials is fine: handles index the material collection)
        objs = np.zeros(n + 1, pkg.OBJECT_DTYPE)
        mats = np.zeros(n_mats, pkg.MATERIAL_DTYPE)
        mats["kind"] = 0
        mats["p"][:, :3] = rng.uniform(0.6, 0.99, (n_mats, 3)).astype(np.float32)  # bright walls: long chains reach the sky
        if n_mats > 2:
            mats["kind"][1] = 1
            mats["p"][1, 3] = 0.1
        objs["center"][:n] = rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32)
        objs["radius"][:n] = rng.uniform(0.4, 1.1, n).astype(np.float32)
        objs["material"][:n] = rng.integers(0, n_mats, n)
        objs["center"][n] = (0.0, -1001.5, 0.0)
        objs["radius"][n] = 1000.0
        objs["material"][n] = n_mats - 1
        kw = dict(aspect_ratio=1.0, image_width=40, samples_per_pixel=12, max_depth=depth, vertical_fov=55.0, defocus_angle=0.0,
                  focus_distance=1.0, lookfrom=(0.0, 1.0, 7.0), lookat=(0.0, 0.0, 0.0), world_up=(0.0, 1.0, 0.0))
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        want, want8 = ob.render_rect_counter(ocam, objs, mats, 17, 0, 0, 40, 40, nthreads=8)
        for accel, _ in _both(pkg):
            with pkg.Scene(cam, objs, mats, accel=accel) as s:
                bits = max(1, int(np.ceil(np.log2(max(2, n_mats)))))
                words = -(-depth // (32 // bits))
                assert s.launch_info()["packed_chains"] == (words + 3) // 4 * 4, (n_mats, depth)
                rgb, rgba = s.render_rows(0, 40, 17)
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8), (n_mats, depth)


def test_random_scenes_and_cameras(pkg, ob, gpu):
    """Forty random worlds -- overlapping and nested spheres, cameras inside spheres, fuzz > 1 (clamped at
    construction), refraction indices below 1, huge and tiny radii, shared material handles -- through both accel
    paths against the oracle."""
    rng = np.random.default_rng(2024)
    for case in range(40):
        n = int(rng.integers(1, 60))
        n_mats = int(rng.integers(1, n + 1))
        objs = np.zeros(n, pkg.OBJECT_DTYPE)
        mats = np.zeros(n_mats, pkg.MATERIAL_DTYPE)
        for m in range(n_mats):
            kind = int(rng.integers(0, 3))
            if kind == 0:
                mats[m] = (0, (*rng.uniform(0.0, 1.0, 3), 0.0))
            elif kind == 1:
                mats[m] = (1, (*rng.uniform(0.3, 1.0, 3), min(1.0, float(rng.uniform(0.0, 1.6)))))
            else:
                mats[m] = (2, (float(rng.uniform(0.6, 2.2)), 0.0, 0.0, 0.0))
        scale = float(rng.choice([0.5, 3.0, 30.0]))
        for i in range(n):
            r = float(rng.choice([0.05, 0.3, 1.0, 4.0, 200.0])) * float(rng.uniform(0.5, 1.5))
            objs[i] = (0, tuple(rng.uniform(-scale, scale, 3)), r, int(rng.integers(0, n_mats)))
        kw = dict(image_width=int(rng.integers(17, 64)), aspect_ratio=float(rng.choice([1.0, 16.0 / 9.0, 2.35])),
                  samples_per_pixel=int(rng.integers(1, 9)), max_depth=int(rng.choice([1, 3, 12, 50])),
                  vertical_fov=float(rng.uniform(10.0, 110.0)), defocus_angle=float(rng.choice([0.0, 0.6, 8.0])),
                  focus_distance=float(rng.uniform(0.5, 12.0)), lookfrom=tuple(rng.uniform(-scale, scale, 3)),
                  lookat=tuple(rng.uniform(-1.0, 1.0, 3)), world_up=(0.0, 1.0, 0.0))
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        if cam.img_height == 0:
            continue
        seed = int(rng.integers(0, 2 ** 62))
        want, want8 = ob.render_rect_counter(ocam, objs, mats, seed, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
        for accel, name in _both(pkg):
            with pkg.Scene(cam, objs, mats, accel=accel) as s:
                rgb, rgba = s.render_rows(0, cam.img_height, seed)
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8), (case, name)


def test_operands_outside_the_range_of_the_division_and_square_root_cores(pkg, ob, gpu):
    """The kernel divides and takes square roots through the in-range cores of the compiler's expansions and falls back
    to the full expansions outside [2^-40, 2^40] (denominators), 2^-60 (numerators) and [2^-90, 2^90] (radicands).
    Worlds scaled by 2^-25 ... 2^+25 put dot(d, d), the discriminants and the radii on both sides of those limits; a
    sphere whose centre coordinates are 2^24 has hit points whose offset from the centre is exactly zero in a component
    (the spacing of fp32 there is 2).  Same frames as the oracle, which divides with `/` and calls sqrtf."""
    rng = np.random.default_rng(77)
    base = [((0.0, -1000.0, 0.0), 1000.0, (0, (0.5, 0.5, 0.5, 0.0)))]
    for _ in range(24):
        k = int(rng.choice([0, 0, 1, 2]))
        prm = ((*rng.uniform(0.1, 0.9, 3), 0.0) if k == 0 else (*rng.uniform(0.5, 1.0, 3), float(rng.uniform(0.0, 0.4))) if k == 1
               else (1.5, 0.0, 0.0, 0.0))
        r = float(rng.choice([0.2, 0.5, 1.0]))
        base.append(((float(rng.uniform(-4, 4)), r, float(rng.uniform(-4, 4))), r, (k, prm)))
    for log2_scale in (-25, -17, 0, 17, 25):
        sc = 2.0 ** log2_scale
        objs, mats = arrays([((c[0] * sc, c[1] * sc, c[2] * sc), r * sc, m) for c, r, m in base])
        kw = dict(image_width=48, samples_per_pixel=4, max_depth=12, vertical_fov=40.0, defocus_angle=0.6,
                  focus_distance=10.0 * sc, lookfrom=(9.0 * sc, 2.0 * sc, 3.0 * sc), lookat=(0.0, 0.5 * sc, 0.0))
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        want, want8 = ob.render_rect_counter(ocam, objs, mats, 5, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
        assert np.isfinite(want).all() and want.max() > 0.0, log2_scale
        for accel, name in _both(pkg):
            with pkg.Scene(cam, objs, mats, accel=accel) as s:
                rgb, rgba = s.render_rows(0, cam.img_height, 5)
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8), (log2_scale, name)
    big = float(2 ** 24)
    objs, mats = arrays([((big, big, big), 1.0, (0, (0.7, 0.3, 0.3, 0.0))), ((big + 4.0, big, big), 2.0, (1, (0.8, 0.8, 0.8, 0.1))),
                         ((big, big - 1002.0, big), 1000.0, (0, (0.5, 0.5, 0.5, 0.0)))])
    kw = dict(image_width=40, samples_per_pixel=8, max_depth=8, vertical_fov=30.0, defocus_angle=0.0, focus_distance=10.0,
              lookfrom=(big + 2.0, big + 2.0, big + 16.0), lookat=(big + 2.0, big, big))
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, want8 = ob.render_rect_counter(ocam, objs, mats, 6, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
    for accel, name in _both(pkg):
        with pkg.Scene(cam, objs, mats, accel=accel) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, 6)
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8), name


def test_degenerate_scenes(pkg, ob, gpu):
    kw = dict(image_width=40, samples_per_pixel=2, max_depth=5)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    lam = (0, (0.5, 0.5, 0.5, 0.0))
    # identical spheres: the first inserted wins every tie (object.defs.cc:73), in the BVH walk too
    dup_spec = [((0.0, 0.0, 0.0), 1.0, (0, (0.9, 0.1, 0.1, 0.0))), ((0.0, 0.0, 0.0), 1.0, (0, (0.1, 0.9, 0.1, 0.0)))] * 6
    for spec in ([], [((0.0, 0.0, 0.0), 1.0, lam)], dup_spec):
        objs, mats = arrays(spec)
        want, _ = ob.render_rect_counter(ocam, objs, mats, 2, 0, 0, ocam.img_width, ocam.img_height)
        for accel, _ in _both(pkg):
            with pkg.Scene(cam, objs, mats, accel=accel) as s:
                rgb, _ = s.render_rows(0, cam.img_height, 2)
            _assert_frames_equal(rgb, want)
    # shared material handles (MaterialCollection is handle-indexed, material.defs.hpp:102-106)
    objs, mats = arrays([((0.0, -100.5, 0.0), 100.0, lam), ((0.0, 0.0, 0.0), 0.5, lam), ((1.0, 0.0, 0.0), 0.5, lam)])
    objs["material"] = [1, 0, 1]
    want, _ = ob.render_rect_counter(ocam, objs, mats, 2, 0, 0, ocam.img_width, ocam.img_height)
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH) as s:
        rgb, _ = s.render_rows(0, cam.img_height, 2)
    _assert_frames_equal(rgb, want)


def _closed_box():
    """The camera sits inside one big Lambertian sphere (every ray hits it from the inside and scatters inwards), a glass
    sphere floats in it: no opening, every path runs until its bounce limit."""
    return arrays([((0.0, 0.0, 0.0), 10.0, (0, (0.8, 0.8, 0.8, 0.0))), ((0.5, -1.0, 0.0), 1.0, (2, (1.5, 0.0, 0.0, 0.0))),
                   ((-2.0, 1.0, -1.0), 1.5, (0, (0.6, 0.7, 0.9, 0.0)))])


def test_inputs_the_reference_api_admits(pkg, ob, gpu):
    """inputs the reference's API accepts that no other test feeds the kernel -- a negative radius (the
    hollow-glass idiom: (p - C) / R flips the normal, object.defs.cc:62-63), radius 0, refraction index exactly 1, fuzz 0
    and fuzz above 1 (Metallic clamps at construction, material.defs.hpp:73; the raw record is passed as is on both
    sides), albedo above 1, center_dist_treshold = 3 (no grid sphere survives `3 > 3`, core.cc:130), lookfrom == lookat
    (a NaN camera), samples_per_pixel = 65535, max_depth = 65535 -- both accel paths, both memory layouts, frames equal
    to the oracle's (NaN = NaN)."""
    lam, glass = (0, (0.5, 0.5, 0.5, 0.0)), (2, (1.5, 0.0, 0.0, 0.0))
    ground = ((0.0, -100.5, 0.0), 100.0, lam)
    worlds = {
        "hollow glass": [ground, ((0.0, 0.0, -1.0), 0.5, glass), ((0.0, 0.0, -1.0), -0.45, glass),
                         ((1.1, 0.0, -1.0), -0.5, (0, (0.8, 0.3, 0.3, 0.0))), ((-1.1, 0.0, -1.0), -0.5, (1, (0.8, 0.8, 0.8, 0.3)))],
        "radius 0": [ground, ((0.0, 0.0, -1.0), 0.0, lam), ((0.3, 0.1, -1.0), 0.0, glass), ((-0.5, 0.0, -1.0), 0.5, lam)],
        "ri 1, fuzz 0 / 1 / 1.6, albedo > 1": [ground, ((0.0, 0.0, -1.0), 0.5, (2, (1.0, 0.0, 0.0, 0.0))),
                                               ((1.0, 0.0, -1.0), 0.5, (1, (0.9, 0.9, 0.9, 0.0))),
                                               ((-1.0, 0.0, -1.0), 0.5, (1, (0.9, 0.6, 0.2, 1.0))),
                                               ((-2.0, 0.0, -1.5), 0.5, (1, (0.7, 0.7, 0.9, 1.6))),
                                               ((2.0, 0.0, -1.5), 0.5, (0, (1.7, 1.2, 3.0, 0.0)))],
    }
    kw = dict(three_spheres_camera(), image_width=64, aspect_ratio=16.0 / 9.0, samples_per_pixel=24, max_depth=12)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    for name, spec in worlds.items():
        objs, mats = arrays(spec)
        want, want8 = ob.render_rect_counter(ocam, objs, mats, 31, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
        assert np.isfinite(want).any(), name
        for accel, _ in _both(pkg):
            for tun in (None, dict(force_hbm_scene=1)):
                with pkg.Scene(cam, objs, mats, accel=accel, tuning=tun) as s:
                    rgb, rgba = s.render_rows(0, cam.img_height, 31)
                _assert_frames_equal(rgb, want)
                assert np.array_equal(rgba, want8), (name, accel, tun)
    # center_dist_treshold = 3: glm's vec3::length() is the component count, so `3 > 3` drops every grid sphere
    objs, mats = pkg.make_world_spheres(12345, wd=pkg.world_def(center_dist_treshold=3.0))
    oobjs, omats = ob.make_world_spheres(12345, wd=ob.world_def(center_dist_treshold=3.0))
    assert len(objs) == 4 and objs.tobytes() == oobjs.tobytes() and mats.tobytes() == omats.tobytes()
    objs29, _ = pkg.make_world_spheres(12345, wd=pkg.world_def(center_dist_treshold=2.9))
    assert len(objs29) == 488
    # lookfrom == lookat: normalize(0) is NaN, every ray is NaN, every pixel is NaN on both sides (black in RGBA8)
    kwn = dict(image_width=24, samples_per_pixel=3, max_depth=5, lookfrom=(1.0, 2.0, 3.0), lookat=(1.0, 2.0, 3.0))
    camn, ocamn = pkg.camera_setup(pkg.camera_params(**kwn)), ob.camera_setup(ob.camera_params(**kwn))
    objs, mats = arrays(worlds["hollow glass"])
    want, want8 = ob.render_rect_counter(ocamn, objs, mats, 5, 0, 0, ocamn.img_width, ocamn.img_height)
    assert np.isnan(want).all()
    for accel, _ in _both(pkg):
        with pkg.Scene(camn, objs, mats, accel=accel) as s:
            rgb, rgba = s.render_rows(0, camn.img_height, 5)
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)
    # samples_per_pixel at the u16 limit on a 2 x 2 image (sample indices 0 .. 65534, one chunked and one whole-pixel launch)
    kws = dict(three_spheres_camera(), image_width=2, aspect_ratio=1.0, samples_per_pixel=65535, max_depth=6)
    cams, ocams = pkg.camera_setup(pkg.camera_params(**kws)), ob.camera_setup(ob.camera_params(**kws))
    objs, mats = three_spheres()
    want, want8 = ob.render_rect_counter(ocams, objs, mats, 77, 0, 0, 2, 2, nthreads=4)
    for accel, _ in _both(pkg):
        for tun in (None, dict(chunk_samples=-1)):
            with pkg.Scene(cams, objs, mats, accel=accel, tuning=tun) as s:
                rgb, rgba = s.render_rows(0, 2, 77)
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8)
    # max_depth at the u16 limit inside a closed sphere: paths bounce thousands of times (fp32 self-intersection lets one
    # leak out to the sky every ~1000 bounces, so none reaches 65535), a lane's attenuation chain can be 65535 entries
    # long and the persistent grid shrinks to what 4 GiB of strips allow
    objs, mats = _closed_box()
    kwd = dict(aspect_ratio=1.0, image_width=2, samples_per_pixel=2, max_depth=65535, vertical_fov=60.0, defocus_angle=0.0,
               focus_distance=1.0, lookfrom=(0.0, 0.0, 3.0), lookat=(0.0, 0.0, 0.0), world_up=(0.0, 1.0, 0.0))
    camd, ocamd = pkg.camera_setup(pkg.camera_params(**kwd)), ob.camera_setup(ob.camera_params(**kwd))
    want, want8, ctr = ob.render_rect_counter(ocamd, objs, mats, 3, 0, 0, 2, 2, nthreads=4, counters=True)
    assert ctr["segments"] > 8 * 500
    for accel, tun in ((pkg.ACCEL_BVH, None), (pkg.ACCEL_BRUTE, None), (pkg.ACCEL_BVH, dict(force_hbm_scene=1))):
        with pkg.Scene(camd, objs, mats, accel=accel, collect_stats=True, tuning=tun) as s:
            rgb, rgba = s.render_rows(0, 2, 3)
            st = s.stats()
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)
        assert st["segments"] == ctr["segments"], st
    # the same box with a limit of 300: most paths end black at the limit (core.cc:238-240), a few leak out
    kwe = dict(kwd, max_depth=300, samples_per_pixel=16, image_width=8)
    came, ocame = pkg.camera_setup(pkg.camera_params(**kwe)), ob.camera_setup(ob.camera_params(**kwe))
    want, want8 = ob.render_rect_counter(ocame, objs, mats, 4, 0, 0, 8, 8, nthreads=8)
    with pkg.Scene(came, objs, mats, accel=pkg.ACCEL_BVH) as s:
        rgb, rgba = s.render_rows(0, 8, 4)
    _assert_frames_equal(rgb, want)
    assert np.array_equal(rgba, want8)


# ---------------------------------------------------------------------------------------------------------------
# boundary behaviour of the C-ABI
# ---------------------------------------------------------------------------------------------------------------
def test_row_ranges_outputs_and_errors(pkg, ob, rtow, gpu):
    kw = dict(image_width=90, samples_per_pixel=2, max_depth=6)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    H = cam.img_height
    want, want8 = ob.render_rect_counter(ocam, *rtow, 6, 0, 0, 90, H, nthreads=8)
    with pkg.Scene(cam, *rtow) as s:
        for y0, y1 in ((0, H), (0, 1), (H - 1, H), (3, 20), (8, 16), (17, 17)):
            rgb, rgba = s.render_rows(y0, y1, 6)
            _assert_frames_equal(rgb, want[y0:y1])
            assert np.array_equal(rgba, want8[y0:y1])
        rgb, none = s.render_rows(0, H, 6, rgba=False)
        assert none is None and rgb.tobytes() == want.tobytes()
        none, rgba = s.render_rows(0, H, 6, rgb=False)
        assert none is None and np.array_equal(rgba, want8)
        for y0, y1 in ((0, H + 1), (5, 4)):
            with pytest.raises(pkg.RtmiError) as e:
                s.render_rows(y0, y1, 6)
            assert e.value.code == pkg.RTMI_ERR_BAD_ARG
        with pytest.raises(pkg.RtmiError):
            s.render_row_blocks_device(H, 8, 1, 1, 6)
    zero = pkg.camera_setup(pkg.camera_params(image_width=64, samples_per_pixel=1))
    zero.samples_per_pixel = 0
    with pytest.raises(pkg.RtmiError) as e:
        pkg.Scene(zero, *rtow)
    assert e.value.code == pkg.RTMI_ERR_BAD_ARG


def test_ragged_image_sizes_chunks_and_block_strides(pkg, ob, gpu):
    """The work-item decode (tile, chunk, pixel, row block: multiply-shift divisions) over awkward geometries: widths and
    heights that are not multiples of the 8x8 tile, sample counts around the chunk size, strided row blocks."""
    torch = gpu
    dev = torch.device("cuda", 0)
    objs, mats = three_spheres()
    rng = np.random.default_rng(99)
    for case in range(36):
        w = int(rng.choice([1, 2, 7, 8, 9, 15, 17, 31, 33, 63, 65, 100]))
        aspect = float(rng.choice([0.5, 1.0, 16.0 / 9.0, 3.0]))
        spp = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33]))
        chunk = int(rng.choice([-1, 1, 2, 3, 4, 5, 8]))
        depth = int(rng.integers(0, 9))
        if int(w / aspect) < 1:
            continue
        kw = dict(three_spheres_camera(), image_width=w, aspect_ratio=aspect, samples_per_pixel=spp, max_depth=depth)
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        W, H = cam.img_width, cam.img_height
        want, want8 = ob.render_rect_counter(ocam, objs, mats, case, 0, 0, W, H)
        with pkg.Scene(cam, objs, mats, tuning=dict(chunk_samples=chunk)) as s:
            rgb, rgba = s.render_rows(0, H, case)
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8), (w, H, spp, chunk)
            block = int(rng.choice([1, 2, 3, 8]))
            world = int(rng.integers(1, 4))
            plan = pkg.RowShardPlan(H, block, world)
            parts = []
            for r in range(world):
                y_first, n_blocks, rows = plan.shard(r)
                buf = torch.zeros((max(1, plan.max_rows), W, 3), dtype=torch.float32, device=dev)
                if n_blocks:
                    s.render_row_blocks_device(y_first, block, world, n_blocks, case, buf.data_ptr(), 0,
                                               torch.cuda.current_stream(dev).cuda_stream)
                parts.append(buf[:plan.max_rows])
            torch.cuda.synchronize()
            frame = torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev)).cpu().numpy()
            _assert_frames_equal(frame, want)


def test_concurrent_calls_on_one_scene(pkg, ob, rtow, gpu):
    """rtmi_render_rows may be called from several host threads on one scene (main.cc:608-611: N workers, one core)."""
    kw = dict(image_width=64, samples_per_pixel=4, max_depth=10)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, _ = ob.render_rect_counter(ocam, *rtow, 7, 0, 0, 64, cam.img_height, nthreads=8)
    res = {}
    with pkg.Scene(cam, *rtow) as s:
        def work(i):
            y0 = i * 9
            res[i] = (y0, s.render_rows(y0, y0 + 9, 7)[0])
        ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    for y0, rgb in res.values():
        _assert_frames_equal(rgb, want[y0:y0 + 9])


def test_device_pointer_entry_and_sharded_blocks(pkg, ob, rtow, gpu):
    """rtmi_render_row_blocks_device with torch-owned HBM buffers on torch's stream; four 'ranks' rendered one after
    the other on this GPU reassemble to the single-GPU frame (the image does not depend on the GPU count)."""
    torch = gpu
    kw = dict(image_width=120, samples_per_pixel=4, max_depth=12)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    want, want8 = ob.render_rect_counter(ocam, *rtow, 21, 0, 0, W, H, nthreads=8)
    dev = torch.device("cuda", 0)
    with pkg.Scene(cam, *rtow, device=0) as s:
        for world in (1, 4, 3):
            plan = pkg.RowShardPlan(H, 8, world)
            parts, parts8 = [], []
            for r in range(world):
                y_first, n_blocks, rows = plan.shard(r)
                rgb = torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev)
                rgba = torch.zeros((plan.max_rows, W), dtype=torch.int32, device=dev)
                s.render_row_blocks_device(y_first, 8, world, n_blocks, 21, rgb.data_ptr(), rgba.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream)
                parts.append(rgb)
                parts8.append(rgba)
            torch.cuda.synchronize()
            assert s.last_kernel_ms() > 0.0
            idx = torch.as_tensor(plan.index, device=dev)
            frame = torch.cat(parts, 0).index_select(0, idx).cpu().numpy()
            frame8 = torch.cat(parts8, 0).index_select(0, idx).cpu().numpy().view(np.uint32)
            _assert_frames_equal(frame, want)
            assert np.array_equal(frame8, want8)


def test_multi_device_frame_entry_degenerate_one_device(pkg, ob, rtow, gpu):
    """rtmi_frame_* with n = 1 (what one box offers): shard plan of one rank, no communicator, de-interleave kernel run
    on the identity map -- the frame must be bit-equal to rtmi_render_rows and to the oracle; also with a block size that
    does not divide the height, and the argument errors of the device list."""
    torch = gpu
    kw = dict(image_width=150, samples_per_pixel=6, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    want, want8 = ob.render_rect_counter(ocam, *rtow, 21, 0, 0, W, H, nthreads=8)
    with pkg.Scene(cam, *rtow) as s:
        ref, ref8 = s.render_rows(0, H, 21)
    _assert_frames_equal(ref, want)
    for block_rows in (8, 5, 0):
        with pkg.Frame(cam, *rtow, devices=(0,), block_rows=block_rows) as f:
            rgb, rgba = f.render(21)
            assert f.rccl_ranks == 0
            t = f.timing()
            assert t["total_ms"] > 0.0 and t["kernel_ms"][0] > 0.0 and t["gather_ms"] >= 0.0
            d_rgb, d_rgba = f.render_device(21)
            assert d_rgb and d_rgba
            torch.cuda.synchronize()
        assert rgb.tobytes() == ref.tobytes() and np.array_equal(rgba, ref8)
    # n > 1 on one box: the rehearsal hook lists the device several times and gathers with copies instead of RCCL; the
    # shard plan (interleaved blocks, ragged last block), the rank-major gather layout and the scanline order are the real ones
    # (tile_order 2: the scenes probe their cost map even for this small frame, so that blocks of whole tile rows are dealt out by
    # cost -- rtmi_shard_plan -- and rendered through rtmi_render_block_list_device; blocks of 5 or 3 rows stay block b -> device b mod n)
    for devices, block_rows, tun in (((0, 0), 8, None), ((0, 0, 0), 5, None), ((0,) * 8, 8, None), ((0,) * 7, 3, None),
                                     ((0, 0), 8, dict(tile_order=2)), ((0,) * 3, 16, dict(tile_order=2)), ((0,) * 8, 8, dict(tile_order=2)),
                                     ((0,) * 3, 5, dict(tile_order=2))):
        with pkg.Frame(cam, *rtow, devices=devices, block_rows=block_rows, rehearsal=True, tuning=tun, cost_plan=tun is not None) as f:
            rgb, rgba = f.render(21)
            assert f.rccl_ranks == 0 and len(f.timing()["kernel_ms"]) == len(devices)
        assert rgb.tobytes() == ref.tobytes() and np.array_equal(rgba, ref8), (devices, block_rows, tun)
    n_dev = torch.cuda.device_count()
    for devices in ((0, 0), (n_dev,), (-1,)):
        with pytest.raises(pkg.RtmiError) as e:
            pkg.Frame(cam, *rtow, devices=devices)
        assert e.value.code == pkg.RTMI_ERR_BAD_ARG
    assert torch.cuda.current_device() == 0  # every entry point restores the caller's device


def test_block_lists_and_the_cost_balanced_shard_plan(pkg, ob, rtow, gpu):
    """row blocks dealt out to the ranks by the scene's cost map (rtmi_shard_plan: longest processing time first, the
    same number of blocks to every rank) and rendered as a LIST (rtmi_render_block_list_device).  Any list gives the rows it names,
    bit for bit -- ascending, shuffled, with the image's clipped last block, in bands, trees in LDS and in HBM -- and the plan made
    from the scene's own probe balances the ranks' costs no worse than block b -> rank b mod N."""
    torch = gpu
    kw = dict(image_width=200, samples_per_pixel=8, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height  # 200 x 112 = 14 blocks of 8 rows
    want, want8 = ob.render_rect_counter(ocam, *rtow, 23, 0, 0, W, H, nthreads=8)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(3)
    for tun in (dict(tile_order=2), dict(tile_order=2, bands=3), dict(force_hbm_scene=1), dict(tile_order=1, chunk_samples=3)):
        with pkg.Scene(cam, *rtow, tuning=tun) as s:
            costs = s.tile_costs()
            assert (costs is not None) == (tun.get("tile_order") == 2)
            for world in (2, 3, 8):
                bc = pkg.block_costs(costs, H, 8) if costs is not None else None
                plan = pkg.CostShardPlan(H, 8, world, bc)
                parts = [torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev) for _ in range(world)]
                parts8 = [torch.zeros((plan.max_rows, W), dtype=torch.int32, device=dev) for _ in range(world)]
                for r in range(world):
                    if len(plan.blocks(r)):
                        s.render_block_list_device(8, plan.blocks(r), 23, parts[r].data_ptr(), parts8[r].data_ptr(), stream)
                torch.cuda.synchronize()
                idx = torch.as_tensor(plan.index, device=dev)
                _assert_frames_equal(torch.cat(parts, 0).index_select(0, idx).cpu().numpy(), want)
                assert np.array_equal(torch.cat(parts8, 0).index_select(0, idx).cpu().numpy().view(np.uint32), want8)
                if bc is not None and world <= 3:
                    loads = [int(bc[plan.blocks(r)].sum()) for r in range(world)]
                    mod = [int(bc[np.arange(len(bc)) % world == r].sum()) for r in range(world)]
                    assert max(loads) <= max(mod), (loads, mod)
            # a shuffled list: the slice holds the blocks in list order
            blocks = rng.permutation(H // 8).astype(np.uint32)[:9]
            buf = torch.zeros((len(blocks) * 8, W, 3), dtype=torch.float32, device=dev)
            s.render_block_list_device(8, blocks, 23, buf.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            for k, b in enumerate(blocks):
                _assert_frames_equal(got[8 * k:8 * k + 8], want[8 * b:8 * b + 8])
            with pytest.raises(pkg.RtmiError) as err:  # tiles must not straddle blocks
                s.render_block_list_device(5, np.array([0, 2], np.uint32), 23, buf.data_ptr(), 0, stream)
            assert err.value.code == pkg.RTMI_ERR_BAD_ARG
            with pytest.raises(pkg.RtmiError) as err:  # a block outside the image
                s.render_block_list_device(8, np.array([0, 99], np.uint32), 23, buf.data_ptr(), 0, stream)
            assert err.value.code == pkg.RTMI_ERR_BAD_ARG
    # an image whose last block is clipped, blocks of 16 rows
    kw = dict(image_width=178, samples_per_pixel=4, max_depth=20)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    assert H % 16 != 0
    want, _ = ob.render_rect_counter(ocam, *rtow, 4, 0, 0, W, H, nthreads=8)
    with pkg.Scene(cam, *rtow, tuning=dict(tile_order=2)) as s:
        plan = pkg.CostShardPlan(H, 16, 3, pkg.block_costs(s.tile_costs(), H, 16))
        parts = [torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev) for _ in range(3)]
        for r in range(3):
            s.render_block_list_device(16, plan.blocks(r), 4, parts[r].data_ptr(), 0, stream)
        torch.cuda.synchronize()
        _assert_frames_equal(torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev)).cpu().numpy(), want)


def test_rccl_runs_with_a_one_rank_communicator(pkg, rtow, gpu):
    """RTMI_FRAME_FORCE_RCCL makes the n = 1 frame do what n > 1 does -- librccl opened at run time,
    ncclCommInitAll, ONE ncclGather per rank inside a group on the render stream (rank 0 gathers its packed float-RGB +
    RGBA8 slice from itself), the de-interleave kernel behind it -- so that the multi-GPU code path has executed before
    the driver's 8-GPU run.  Frame bit-equal to rtmi_render_rows, also twice in a row and with a ragged block size."""
    torch = gpu
    kw = dict(image_width=150, samples_per_pixel=6, max_depth=50)
    cam = pkg.camera_setup(pkg.camera_params(**kw))
    H = cam.img_height
    with pkg.Scene(cam, *rtow) as s:
        ref, ref8 = s.render_rows(0, H, 21)
        ref_b, _ = s.render_rows(0, H, 22)
    for block_rows in (8, 5):
        with pkg.Frame(cam, *rtow, devices=(0,), block_rows=block_rows, force_rccl=True) as f:
            assert f.rccl_ranks == 1
            rgb, rgba = f.render(21)
            t = f.timing()
            assert t["gather_ms"] > 0.0 and t["kernel_ms"][0] > 0.0
            rgb_b, _ = f.render(22)
            rgb_c, rgba_c = f.render(21)
        assert rgb.tobytes() == ref.tobytes() and np.array_equal(rgba, ref8)
        assert rgb_b.tobytes() == ref_b.tobytes()
        assert rgb_c.tobytes() == ref.tobytes() and np.array_equal(rgba_c, ref8)
    assert torch.cuda.current_device() == 0


def test_bench_force_dist_runs_the_rccl_process_group_with_one_rank(gpu):
    """`bench.py --gpus 1 --force-dist`: the launcher starts one rank under torch.distributed.run before anything touches
    the GPU, the rank initialises the "nccl" (RCCL) process group and sends its frame through the gather collective and
    the timing all-reduce with world size 1; `--single-process --force-dist` does the same inside librtmi.so."""
    import subprocess
    import sys
    from tests.conftest import ROOT
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--config", "2", "--width", "160",
            "--spp", "8", "--steps", "2", "--warmup", "0", "--full", "--no-cpu-baseline", "--no-linear-scan"]
    for extra in ([], ["--single-process"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert doc["rccl_ranks"] == 1 and doc["n_gpus"] == 1 and doc["value"] > 0, doc
        if not extra:
            assert doc["parity_check"]["max_abs_diff_vs_oracle"] == 0.0 and "nccl" in doc["config"]["launcher"]


def test_bench_plain_run_times_the_steps_and_dumps_the_last_frame(pkg, gpu, tmp_path):
    """A plain `bench.py` run (no --full) prints the headline and nothing that needs work of its own; `--dump-outputs DIR`
    writes the frame of the last timed step, which is the frame rtmi_render_rows gives for the same scene and seed -- through
    the torch path and through rtmi_frame_* (`--single-process`)."""
    import subprocess
    import sys
    from tests.conftest import ROOT
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--width", "160", "--spp", "8",
            "--steps", "3", "--warmup", "1"]
    kw = dict(image_width=160, samples_per_pixel=8, max_depth=50)
    cam = pkg.camera_setup(pkg.camera_params(**kw))
    with pkg.Scene(cam, *pkg.make_world_spheres(12345), accel=pkg.ACCEL_BVH) as s:
        want, want8 = s.render_rows(0, cam.img_height, 2025)  # (bench.py's SCENE_SEED and RENDER_SEED)
    for extra in ([], ["--single-process"]):
        out = tmp_path / ("dump" + "".join(extra))
        r = subprocess.run(base + extra + ["--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        doc = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in doc, k
        assert doc["steps"] == 3 and doc["warmup"] == 1 and doc["ms_per_step"] > 0 and doc["value"] > 0
        for k in ("value_e2e", "parity_check", "roofline", "linear_scan_kernel", "cpu_baseline"):
            assert k not in doc, k
        assert doc["dumped_outputs"]["files"] == ["rgb.npy", "rgba8.npy"]
        rgb, rgba8 = np.load(out / "rgb.npy"), np.load(out / "rgba8.npy")
        assert rgb.dtype == np.float32 and rgba8.dtype == np.float32
        assert rgb.shape == want.shape and rgba8.shape == want.shape[:2] + (4,)
        assert rgb.tobytes() == want.tobytes()
        assert np.array_equal(rgba8.astype(np.uint8), want8.view(np.uint8).reshape(rgba8.shape))


def test_multi_device_frame_over_rccl(pkg, rtow, gpu):
    """the real n > 1 path -- one rank per device, ncclCommInitAll(n), the grouped gather over xGMI -- on boxes
    that have more than one GPU (skipped on the one-GPU box): frame bit-equal to rtmi_render_rows, rccl_ranks == n."""
    torch = gpu
    n_dev = torch.cuda.device_count()
    if n_dev < 2:
        pytest.skip("one visible GPU: RCCL with n > 1 needs one device per rank")
    kw = dict(image_width=200, samples_per_pixel=8, max_depth=50)
    cam = pkg.camera_setup(pkg.camera_params(**kw))
    with pkg.Scene(cam, *rtow, device=0) as s:
        ref, ref8 = s.render_rows(0, cam.img_height, 5)
    for n in sorted({2, min(n_dev, 6)}):  # (the box allows six processes / contexts on its cards)
        with pkg.Frame(cam, *rtow, devices=tuple(range(n)), block_rows=8) as f:
            assert f.rccl_ranks == n
            rgb, rgba = f.render(5)
            rgb2, _ = f.render(5)
        assert rgb.tobytes() == ref.tobytes() and np.array_equal(rgba, ref8) and rgb2.tobytes() == ref.tobytes(), n
    # the bench harness over the same path: one process driving two devices (rtmi_frame_*), and two ranks under
    # torch.distributed.run with the "nccl" backend
    import subprocess
    import sys
    from tests.conftest import ROOT
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "2", "--width", "200", "--spp", "8",
            "--steps", "2", "--warmup", "0", "--no-cpu-baseline", "--no-linear-scan"]
    for extra in (["--single-process"], []):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert doc["rccl_ranks"] == 2 and doc["n_gpus"] == 2 and doc["value"] > 0, doc


def test_scene_just_below_the_lds_limit_keeps_two_workgroups_per_cu(pkg, gpu):
    """the LDS-residency test and the carve-up use one expression: a scene whose staged size lands within a
    kilobyte of 80 KiB either stays in HBM or still runs two workgroups per CU -- never one."""
    cam = pkg.camera_setup(pkg.camera_params(image_width=32, samples_per_pixel=1, max_depth=4))
    seen_lds = seen_hbm = False
    for n in range(480, 800, 2):
        objs, mats = random_spheres(n, seed=3)
        with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH) as s:
            li = s.launch_info()
        if li["scene_in_lds"]:
            seen_lds = True
            assert li["lds_bytes"] <= 80 * 1024 and li["blocks_per_cu"] == 2, (n, li)
        else:
            seen_hbm = True
    assert seen_lds and seen_hbm  # the sweep crossed the limit


def test_images_wider_than_16_bit_coordinates(pkg, ob, gpu):
    """Pixel indices are 32-bit everywhere (round 1 packed x | y << 16 into its deferred-path records): 70000 x 8."""
    objs, mats = three_spheres()
    kw = dict(three_spheres_camera(), image_width=70000, aspect_ratio=70000.0 / 8.0, samples_per_pixel=8, max_depth=24)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    assert (cam.img_width, cam.img_height) == (70000, 8)
    want, want8 = ob.render_rect_counter(ocam, objs, mats, 3, 0, 0, 70000, 8, nthreads=8)
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, tuning=dict(chunk_samples=2)) as s:
        rgb, rgba = s.render_rows(0, 8, 3)
    _assert_frames_equal(rgb, want)
    assert np.array_equal(rgba, want8)


def test_frames_larger_than_the_sample_buffer_are_rendered_in_bands(pkg, ob, rtow, gpu):
    """When the sample records of a call exceed rtmi_tuning::sample_buf_mb the call is split into bands of rows (contiguous
    rows) or of whole row blocks (sharded call); the draw streams are keyed by the absolute pixel, so the frame is the
    oracle's, bit for bit, and rtmi_scene_last_kernel_ms brackets all bands."""
    torch = gpu
    kw = dict(image_width=128, samples_per_pixel=96, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    want, want8 = ob.render_rect_counter(ocam, *rtow, 45, 0, 0, W, H, nthreads=8)
    # 196 KB of records per row: 5 rows per band
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, tuning=dict(sample_buf_mb=1)) as s:
        rgb, rgba = s.render_rows(0, H, 45)
        assert s.last_kernel_ms() > 0.0
        part, part8 = s.render_rows(7, 31, 45)  # a row range that is not a multiple of the band
    _assert_frames_equal(rgb, want)
    assert np.array_equal(rgba, want8)
    _assert_frames_equal(part, want[7:31])
    assert np.array_equal(part8, want8[7:31])
    dev = torch.device("cuda", 0)
    with pkg.Scene(cam, *rtow, device=0, tuning=dict(sample_buf_mb=4)) as s:  # 21 rows: two 8-row blocks per band
        plan = pkg.RowShardPlan(H, 8, 2)
        parts = []
        for r in range(2):
            y_first, n_blocks, rows = plan.shard(r)
            buf = torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev)
            s.render_row_blocks_device(y_first, 8, 2, n_blocks, 45, buf.data_ptr(), 0,
                                       torch.cuda.current_stream(dev).cuda_stream)
            parts.append(buf)
        torch.cuda.synchronize()
        frame = torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev)).cpu().numpy()
    _assert_frames_equal(frame, want)


def test_render_rect_tiles_the_frame(pkg, ob, rtow, gpu):
    """rtmi_render_rect / rtmi_render_rect_device (0.5): the reference's seam is a tile, RayTracingWorkPackage{start, end}
    (main.cc:404-407, consumed pixel by pixel at :507-519).  A frame rendered as shuffled 8x8 packages -- the reference's own
    queue, main.cc:615-633 -- and as 64x16 tiles equals rtmi_render_rows and the oracle bit for bit (the draw streams are keyed
    by the absolute pixel), on both accel paths, both memory layouts, both chain forms; clipped tiles at the right and bottom
    edges (120 x 67 is a multiple of neither tile size); the error paths."""
    torch = gpu
    rng = np.random.default_rng(5)
    for kw, accel, tun in ((dict(image_width=120, samples_per_pixel=12, max_depth=50), pkg.ACCEL_BVH, None),
                           (dict(image_width=120, samples_per_pixel=12, max_depth=12), pkg.ACCEL_BRUTE, None),  # packed chains
                           (dict(image_width=120, samples_per_pixel=3, max_depth=50), pkg.ACCEL_BVH, dict(force_hbm_scene=1))):  # whole-pixel items
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        W, H = cam.img_width, cam.img_height
        want, want8 = ob.render_rect_counter(ocam, *rtow, 77, 0, 0, W, H, nthreads=8)
        with pkg.Scene(cam, *rtow, accel=accel, tuning=tun) as s:
            rows, rows8 = s.render_rows(0, H, 77)
            _assert_frames_equal(rows, want)
            assert np.array_equal(rows8, want8)
            for tw, th in ((8, 8), (64, 16)):
                tiles = [(x, y) for y in range(0, H, th) for x in range(0, W, tw)]
                rng.shuffle(tiles)
                got, got8 = np.zeros_like(rows), np.zeros_like(rows8)
                for x, y in tiles:
                    x1, y1 = min(W, x + tw), min(H, y + th)
                    t, t8 = s.render_rect(x, y, x1, y1, 77)
                    assert t.shape == (y1 - y, x1 - x, 3) and t8.shape == (y1 - y, x1 - x)
                    got[y:y1, x:x1], got8[y:y1, x:x1] = t, t8
                _assert_frames_equal(got, rows)
                assert np.array_equal(got8, rows8)
            # either output alone, an empty rectangle, a one-pixel one
            only8 = s.render_rect(3, 5, 40, 21, 77, rgb=False)[1]
            assert np.array_equal(only8, rows8[5:21, 3:40])
            e, e8 = s.render_rect(9, 9, 9, 30, 77)
            assert e.shape == (21, 0, 3) and e8.shape == (21, 0)
            one, _ = s.render_rect(W - 1, H - 1, W, H, 77)
            _assert_frames_equal(one, rows[H - 1:, W - 1:])
            # device-pointer form, asynchronous on the caller's stream
            dev = torch.device("cuda", 0)
            buf = torch.zeros((30, 50, 3), dtype=torch.float32, device=dev)
            buf8 = torch.zeros((30, 50), dtype=torch.int32, device=dev)
            s.render_rect_device(33, 20, 83, 50, 77, buf.data_ptr(), buf8.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            _assert_frames_equal(buf.cpu().numpy(), rows[20:50, 33:83])
            assert np.array_equal(buf8.cpu().numpy().view(np.uint32), rows8[20:50, 33:83])
            for bad in ((0, 0, W + 1, 8), (0, 0, 8, H + 1), (9, 0, 8, 8), (0, 9, 8, 8)):
                with pytest.raises(pkg.RtmiError) as err:
                    s.render_rect(*bad, 77)
                assert err.value.code == pkg.RTMI_ERR_BAD_ARG


def test_cost_ordered_tiles_and_sequential_bands_do_not_change_the_image(pkg, ob, rtow, gpu):
    """Scheduling: the 8x8 tiles of a launch handed out costliest first (per-tile segment counts from one probe launch per
    scene), and a call rendered in bands of rows (rtmi_tuning::bands), one launch sequence after the other on the caller's
    stream.  Neither changes a bit: whole frames, row ranges that
    do not start on a tile row, sharded row blocks, rectangles, both accel paths, packed and run-length chains; the launch
    report says what the most recent call did; back-to-back asynchronous calls on one stream stay ordered."""
    torch = gpu
    kw = dict(image_width=160, samples_per_pixel=24, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    want, want8 = ob.render_rect_counter(ocam, *rtow, 46, 0, 0, W, H, nthreads=8)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for accel, _ in _both(pkg):
        for tun in (dict(tile_order=2), dict(tile_order=2, bands=4), dict(tile_order=1, bands=3, chunk_samples=5),
                    dict(tile_order=2, bands=2, force_hbm_scene=1), dict(tile_order=2, bands=5, chain_mode=1, block_lanes=512),
                    dict(tile_order=2, chunk_samples=7, bands=2)):
            with pkg.Scene(cam, *rtow, accel=accel, tuning=tun) as s:
                assert s.launch_info()["bands"] == 0
                rgb, rgba = s.render_rows(0, H, 46)
                li = s.launch_info()
                assert li["bands"] == min(tun.get("bands", 1), 4) and li["tile_order"] == (1 if tun["tile_order"] == 2 else 0), (tun, li)
                assert (li["probe_us"] > 0) == (tun["tile_order"] == 2)
                assert s.last_kernel_ms() > 0.0
                _assert_frames_equal(rgb, want)
                assert np.array_equal(rgba, want8)
                part, part8 = s.render_rows(5, 77, 46)  # bands of whole tile rows from a row that is not a multiple of 8
                _assert_frames_equal(part, want[5:77])
                assert np.array_equal(part8, want8[5:77])
                rect, _ = s.render_rect(13, 3, 150, 88, 46)
                _assert_frames_equal(rect, want[3:88, 13:150])
                # three ranks' worth of interleaved row blocks, launched back to back on one stream without a host sync in between
                plan = pkg.RowShardPlan(H, 8, 3)
                parts = [torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev) for _ in range(3)]
                for r in range(3):
                    y_first, n_blocks, _rows = plan.shard(r)
                    s.render_row_blocks_device(y_first, 8, 3, n_blocks, 46, parts[r].data_ptr(), 0, stream)
                torch.cuda.synchronize()
                frame = torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev)).cpu().numpy()
                _assert_frames_equal(frame, want)
    # the box of config 5 (packed chains multiplied by the resolve pass) in six sequential bands
    g = np.load(os.path.join(GOLDEN, "cornell_counter_48x48x32.npz"))
    ccam = pkg.camera_setup(pkg.camera_params(**json.loads(str(g["camera"]))))
    with pkg.Scene(ccam, g["objects"], g["materials"], tuning=dict(tile_order=2, bands=6)) as s:
        rgb, rgba = s.render_rows(0, ccam.img_height, int(g["seed"]))
        assert s.launch_info()["bands"] == 6 and s.launch_info()["packed_chains"] > 0
    _assert_frames_equal(rgb, g["rgb"])
    assert np.array_equal(rgba, g["rgba"])
    with pytest.raises(pkg.RtmiError) as err:
        pkg.Scene(cam, *rtow, tuning=dict(tile_order=3))
    assert err.value.code == pkg.RTMI_ERR_BAD_ARG


def test_walk_starts_of_scattered_rays_do_not_change_the_image(pkg, ob, rtow, gpu):
    """rtmi_tuning::walk_start (0.6): on trees that stay in HBM the walk of a scattered ray starts in the leaf of the sphere it was
    scattered off, the way above it pre-loaded on the stack (host data: tests/test_host_cpu.py::test_walk_starts_keep_the_walk_exact).
    Same frame as the oracle's linear scan with it on (default) and off, with and without camera entries and the staged top of the
    tree, whole-pixel items, both pad rules; and exactly the box and sphere tests of the oracle's walk that follows the same
    records -- fewer than from the root."""
    worlds = [(*rtow, dict(image_width=160, samples_per_pixel=6, max_depth=50))]
    objs, mats, kw = big_grid(90, seed=6)
    worlds.append((objs, mats, dict(kw, image_width=128, samples_per_pixel=4, max_depth=30)))
    for objs, mats, kw in worlds:
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        W, H = cam.img_width, cam.img_height
        want, want8 = ob.render_rect_counter(ocam, objs, mats, 17, 0, 0, W, H, nthreads=8)
        tests = {}
        for tun in (dict(), dict(walk_start=1), dict(cam_entry=2), dict(lds_top_nodes=1), dict(chunk_samples=-1, pad_mode=1),
                    dict(pad_mode=2, lds_top_nodes=9, block_lanes=512)):
            with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, collect_stats=True, tuning=dict(tun, force_hbm_scene=1)) as s:
                li = s.launch_info()
                assert li["scene_in_lds"] == 0 and li["walk_start"] == (0 if tun.get("walk_start") else 1), (tun, li)
                rgb, rgba = s.render_rows(0, H, 17)
                st = s.stats()
                bvh = s.bvh()
                assert (bvh["walk_starts"] is not None) == (li["walk_start"] == 1)
                _assert_frames_equal(rgb, want)
                assert np.array_equal(rgba, want8)
                if tun in (dict(), dict(walk_start=1), dict(cam_entry=2)):
                    ob.set_pad_mode(li["pad_mode"])
                    try:
                        _, _, c = ob.render_rect_counter(ocam, objs, mats, 17, 0, 0, W, H, nthreads=8, counters=True, bvh=bvh)
                    finally:
                        ob.set_pad_mode(0)
                    assert st["segments"] == c["segments"]
                    assert abs(st["node_tests"] - c["node_tests"]) <= 1e-3 * c["node_tests"], (tun, st, c)
                    assert abs(st["sphere_tests"] - c["sphere_tests"]) <= 1e-3 * c["sphere_tests"], (tun, st, c)
                    tests[tun.get("walk_start", 0)] = st["node_tests"]
                part, _ = s.render_rows(3, 50, 17)
                _assert_frames_equal(part, want[3:50])
        assert tests[0] < 0.9 * tests[1], tests
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH) as s:  # trees staged into LDS have no room for the records
        assert s.launch_info()["walk_start"] == 0 and s.bvh()["walk_starts"] is None


def test_record_buffers_of_several_scenes_never_exceed_the_device(pkg, rtow, gpu):
    """scenes keep their sample-record buffers between calls, and the cap on one band's records used to come from the
    device's TOTAL memory (a third of it), whatever else lived there.  Several scenes on one device whose record buffers together
    exceed it: every frame must still come out (the later scenes in more, smaller bands, or with whole-pixel work items), bit
    for bit the same, or the library must answer RTMI_ERR_OOM -- it never aborts (include/rtmi.h: "never throws, never aborts")."""
    import hashlib
    torch = gpu
    _free, total = torch.cuda.mem_get_info(0)
    kw = dict(image_width=1920, samples_per_pixel=2048, max_depth=50)
    cam = pkg.camera_setup(pkg.camera_params(**kw))
    per_scene = cam.img_width * cam.img_height * 2048 * 16  # 68 GB of records for the frame in one band
    n = int(total // per_scene) + 2
    scenes, digests, bands = [], [], []
    try:
        for i in range(n):
            try:
                s = pkg.Scene(cam, *rtow)
                scenes.append(s)
                _, rgba = s.render_rows(0, cam.img_height, 11, rgb=False)
            except pkg.RtmiError as e:
                assert e.code == pkg.RTMI_ERR_OOM, e
                continue
            li = s.launch_info()
            digests.append(hashlib.sha256(rgba.tobytes()).hexdigest())
            bands.append((li["bands"], li["whole_pixel_fallbacks"], li["reband_retries"]))
        assert len(digests) >= 2 and len(set(digests)) == 1, (digests, bands)
        assert bands[0][0] == 1 and (bands[-1][0] > 1 or bands[-1][1] > 0 or len(digests) < n), bands
    finally:
        for s in scenes:
            s.close()


def test_camera_entries_do_not_change_the_image(pkg, ob, rtow, gpu):
    """rtmi_tuning::cam_entry (0.6): the walks of camera rays start at their image tile's entry (host table, see
    tests/test_host_cpu.py::test_camera_tile_entries_keep_the_walk_exact) instead of the root.  Same frame as the oracle's linear
    scan with the table on (default) and off, trees in LDS and in HBM, whole-pixel items, rows and rectangles that do not start on
    a tile (the table is indexed by the ABSOLUTE pixel), sharded row blocks; fewer box tests with it, and exactly the box and sphere
    tests of the oracle's walk that follows the same table."""
    kw = dict(image_width=200, samples_per_pixel=6, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    want, want8 = ob.render_rect_counter(ocam, *rtow, 61, 0, 0, W, H, nthreads=8)
    tests = {}
    for tun in (dict(), dict(cam_entry=1), dict(force_hbm_scene=1), dict(force_hbm_scene=1, cam_entry=1), dict(force_hbm_scene=1, walk_start=1),
                dict(force_hbm_scene=1, walk_start=1, cam_entry=2), dict(chunk_samples=-1), dict(tile_order=2, bands=3),
                dict(chain_mode=1, block_lanes=512)):
        with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, collect_stats=True, tuning=tun or None) as s:
            # (default: trees in LDS, and trees in HBM whose scattered rays start in their own leaf)
            on = tun.get("cam_entry", 0) == 2 or (tun.get("cam_entry", 0) == 0 and not (tun.get("force_hbm_scene") and tun.get("walk_start")))
            li = s.launch_info()
            assert li["cam_entry"] == (1 if on else 0) and (li["entry_build_us"] > 0) == on, (tun, li)
            rgb, rgba = s.render_rows(0, H, 61)
            st = s.stats()
            _assert_frames_equal(rgb, want)
            assert np.array_equal(rgba, want8)
            bvh = s.bvh()
            assert (bvh["entries"] is not None) == on
            if tun == dict() or tun == dict(cam_entry=1) or "force_hbm_scene" in tun:
                _, _, c = ob.render_rect_counter(ocam, *rtow, 61, 0, 0, W, H, nthreads=8, counters=True, bvh=bvh)
                assert st["segments"] == c["segments"]
                assert abs(st["node_tests"] - c["node_tests"]) <= 1e-3 * c["node_tests"], (tun, st, c)
                assert abs(st["sphere_tests"] - c["sphere_tests"]) <= 1e-3 * c["sphere_tests"], (tun, st, c)
                if not tun.get("walk_start"):
                    tests[on, "force_hbm_scene" in tun] = st["node_tests"]
            part, _ = s.render_rows(5, 77, 61)
            _assert_frames_equal(part, want[5:77])
            rect, _ = s.render_rect(13, 3, 150, 88, 61)
            _assert_frames_equal(rect, want[3:88, 13:150])
    assert tests[True, False] < 0.9 * tests[False, False] and tests[True, True] < 0.9 * tests[False, True], tests
    # a table that says "no walk" for the sky and a leaf for a lone sphere: one sphere over a ground, seen from afar
    objs, mats = arrays([((0.0, -1000.0, 0.0), 1000.0, (0, (0.5, 0.5, 0.5, 0.0))), ((0.0, 1.0, 0.0), 1.0, (2, (1.5, 0.0, 0.0, 0.0))),
                         ((-3.0, 0.4, 1.0), 0.4, (1, (0.8, 0.7, 0.6, 0.2))), ((2.5, 0.3, -1.0), 0.3, (0, (0.2, 0.5, 0.7, 0.0)))] +
                        [((0.7 * i - 6.0, 0.15, 3.0 + 0.1 * (i % 3)), 0.15, (i % 3, (0.6, 0.6, 0.6, 0.1) if i % 3 != 2 else (1.4, 0, 0, 0))) for i in range(30)])
    kw = dict(image_width=120, samples_per_pixel=5, max_depth=20, defocus_angle=1.5)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    want, _ = ob.render_rect_counter(ocam, objs, mats, 3, 0, 0, cam.img_width, cam.img_height, nthreads=8)
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH) as s:
        ent = s.bvh()["entries"]
        assert (ent == 0xffffffff).any() and ((ent & 0x80000000) != 0).any()
        rgb, _ = s.render_rows(0, cam.img_height, 3)
    _assert_frames_equal(rgb, want)


def test_differential_fuzz_slice(pkg, ob, gpu):
    """A slice of tools/fuzz_vs_oracle.py where the driver runs it (the round-4 log of 9 800 worlds is
    profiles/r04_fuzz_vs_oracle.txt): 200 random worlds -- 1-90 spheres, every fourth 100-600 spheres over a field hundreds of
    radii wide; negative radii, scales 1e-2 .. 1e3, bounce limits up to 120 -- through the walk x {LDS, HBM with the top of the
    tree staged / not staged, either pad rule, run-length chains, whole-pixel items, cost-ordered tiles in three sequential bands}
    and the scan x 4 variants, every float against the oracle (NaN = NaN)."""
    rng = np.random.default_rng(505)
    bad = []
    for case in range(200):
        objs, mats, kw = pkg.workloads.fuzz_world(rng, case)
        cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
        want, want8 = ob.render_rect_counter(ocam, objs, mats, case, 0, 0, ocam.img_width, ocam.img_height, nthreads=8)
        for accel in (pkg.ACCEL_BVH, pkg.ACCEL_BRUTE):
            tunings = (None, dict(force_hbm_scene=1, chain_mode=1), dict(chunk_samples=-1), dict(tile_order=2, bands=3, chunk_samples=2))
            if accel == pkg.ACCEL_BVH:  # (two of the four walk-only variants per world)
                tunings += ((dict(pad_mode=2), dict(pad_mode=1, force_hbm_scene=1, lds_top_nodes=10, bvh_passes=9)) if case % 2 else
                            (dict(pad_mode=1, bvh_passes=1), dict(pad_mode=2, force_hbm_scene=1, lds_top_nodes=1)))
            for tun in tunings:
                with pkg.Scene(cam, objs, mats, accel=accel, tuning=tun) as s:
                    rgb, rgba = s.render_rows(0, cam.img_height, case)
                same = (rgb.view(np.uint32) == want.view(np.uint32)) | (np.isnan(rgb) & np.isnan(want))
                if not same.all() or not np.array_equal(rgba, want8):
                    bad.append((case, accel, tun, int((~same).any(-1).sum())))
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", ["thumb_config2", "thumb_config5"])
def test_regression_thumbnails(pkg, gpu, name):
    """The stored regression images (tests/golden/thumb_*.png, written by the oracle) against the GPU's RGBA8 output."""
    from tests.golden.make_thumbnails import SEED, read_png, rgba_to_rgb, thumbs
    objs, mats, kw = thumbs()[name]
    cam = pkg.camera_setup(pkg.camera_params(**kw))
    with pkg.Scene(cam, objs, mats) as s:
        _, rgba = s.render_rows(0, cam.img_height, SEED)
    assert np.array_equal(rgba_to_rgb(rgba), read_png(os.path.join(GOLDEN, name + ".png")))


def test_box_pad_rules_count_the_same_tests_as_the_oracle_walk(pkg, ob, gpu):
    """The two pad rules of DESIGN.md 5.4 (rtmi_tuning::pad_mode 1 / 2; 0 = the library's choice: refined on the wide grid,
    class pad on S-RTOW) on the GPU against the oracle's instrumented walk under the same rule: same frame, same segments,
    box and sphere tests within 1e-3 (v_rcp_f32 / v_sqrt_f32 against true division and sqrtf)."""
    worlds = []
    objs, mats, kw = big_grid(120, seed=4)
    worlds.append((objs, mats, dict(kw, image_width=96, samples_per_pixel=4, max_depth=30), 2))
    objs, mats = pkg.make_world_spheres(4242)
    worlds.append((objs, mats, dict(image_width=96, samples_per_pixel=4, max_depth=50), 1))
    try:
        for objs, mats, kw, auto_is in worlds:
            cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
            counts = {}
            for mode in (1, 2, 0):
                for hbm in (0, 1):
                    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, collect_stats=True,
                                   tuning=dict(pad_mode=mode, force_hbm_scene=hbm)) as s:
                        rgb, _ = s.render_rows(0, cam.img_height, 31)
                        st = s.stats()
                        bvh = s.bvh()
                    ob.set_pad_mode(mode)
                    want, _, c = ob.render_rect_counter(ocam, objs, mats, 31, 0, 0, ocam.img_width, ocam.img_height, nthreads=8,
                                                        counters=True, bvh=bvh)
                    _assert_frames_equal(rgb, want)
                    assert st["segments"] == c["segments"]
                    assert abs(st["node_tests"] - c["node_tests"]) <= 1e-3 * c["node_tests"], (mode, hbm)
                    assert abs(st["sphere_tests"] - c["sphere_tests"]) <= 1e-3 * c["sphere_tests"], (mode, hbm)
                    counts[mode, hbm] = c["node_tests"]
            assert counts[0, 0] == counts[auto_is, 0] and counts[2, 0] <= counts[1, 0]
    finally:
        ob.set_pad_mode(0)


def test_kernel_statistics_match_oracle_counters(pkg, ob, rtow, gpu):
    kw = dict(image_width=96, samples_per_pixel=8, max_depth=50)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH, collect_stats=True) as s:
        s.render_rows(0, cam.img_height, 5)
        st = s.stats()
        bvh = s.bvh()
    _, _, c = ob.render_rect_counter(ocam, *rtow, 5, 0, 0, 96, cam.img_height, nthreads=8, counters=True, bvh=bvh)
    assert st["samples"] == c["samples"] == 96 * cam.img_height * 8
    assert st["segments"] == c["segments"]
    # the GPU uses v_rcp_f32 for 1/d in the (conservative) slab test, the oracle a true division: visit counts may
    # differ in the last digits, the image may not
    assert abs(st["node_tests"] - c["node_tests"]) <= 1e-3 * c["node_tests"]
    assert abs(st["sphere_tests"] - c["sphere_tests"]) <= 1e-3 * c["sphere_tests"]
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BRUTE, collect_stats=True) as s:
        s.render_rows(0, cam.img_height, 5)
        st = s.stats()
    assert st["segments"] == c["segments"] and st["sphere_tests"] == 488 * c["segments"] and st["node_tests"] == 0


def test_leaves_peeled_off_the_top_of_the_tree(pkg, ob, gpu):
    """Scenes whose BVH starts with a spine of (leaf | subtree) nodes -- one to four huge spheres around a cluster, and
    trees that are nothing but a spine -- are tested at segment set-up instead of being walked; image and counters must
    still be the oracle's (its walk peels the same leaves)."""
    lam = (0, (0.6, 0.5, 0.4, 0.0))
    cluster = [((0.3 * i - 1.0, 0.2, 0.25 * j - 0.5), 0.1, (i % 3, (0.7, 0.6, 0.5, 0.1) if i % 3 != 2 else (1.5, 0.0, 0.0, 0.0)))
               for i in range(6) for j in range(4)]
    walls = [((0.0, -1000.0, 0.0), 1000.0, lam), ((0.0, 0.0, -1030.0), 1000.0, lam), ((-1030.0, 0.0, 0.0), 1000.0, lam),
             ((1030.0, 0.0, 0.0), 1000.0, lam), ((0.0, 1040.0, 0.0), 1000.0, lam)]
    kw = dict(image_width=96, samples_per_pixel=6, max_depth=20, vertical_fov=40.0, defocus_angle=0.0, focus_distance=5.0,
              lookfrom=(0.0, 1.0, 6.0), lookat=(0.0, 0.2, 0.0), world_up=(0.0, 1.0, 0.0), aspect_ratio=1.5)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    for n_walls, n_cluster in ((1, 24), (2, 24), (3, 24), (5, 24), (2, 0), (3, 1), (4, 0), (1, 1)):
        objs, mats = arrays(walls[:n_walls] + cluster[:n_cluster])
        bvh = pkg.bvh_build(objs)
        bvh = dict(bvh, nodes=bvh["nodes"].view(ob.BVH_NODE_DTYPE), entries=pkg.tile_entries_build(cam, objs))  # (what the scene does)
        want, want8, c = ob.render_rect_counter(ocam, objs, mats, 9, 0, 0, ocam.img_width, ocam.img_height, counters=True,
                                                bvh=bvh, nthreads=8)
        with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, collect_stats=True) as s:
            rgb, rgba = s.render_rows(0, cam.img_height, 9)
            st = s.stats()
        _assert_frames_equal(rgb, want)
        assert np.array_equal(rgba, want8)
        assert st["segments"] == c["segments"], (n_walls, n_cluster)
        assert abs(st["sphere_tests"] - c["sphere_tests"]) <= 1e-3 * c["sphere_tests"] + 2
        assert abs(st["node_tests"] - c["node_tests"]) <= 1e-3 * c["node_tests"] + 2


# ---------------------------------------------------------------------------------------------------------------
# BASELINE.json's full sizes: size-independent properties
# ---------------------------------------------------------------------------------------------------------------
def test_config2_full_frame_properties(pkg, ob, rtow, gpu):
    """config 2: RTOW final scene 1200x675, 100 spp, 50 bounces."""
    cam = pkg.camera_setup(pkg.camera_params(image_width=1200, samples_per_pixel=100, max_depth=50))
    ocam = ob.camera_setup(ob.camera_params(image_width=1200, samples_per_pixel=100, max_depth=50))
    H = cam.img_height
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH) as s:
        full, full8 = s.render_rows(0, H, 2025)
        again, _ = s.render_rows(0, H, 2025)
        assert again.tobytes() == full.tobytes()  # deterministic
        part, _ = s.render_rows(301, 340, 2025)
        assert part.tobytes() == full[301:340].tobytes()  # a row range is a slice of the frame
        other, _ = s.render_rows(301, 309, 2026)
        assert other.tobytes() != full[301:309].tobytes()  # the seed matters
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BRUTE) as s:
        brute, brute8 = s.render_rows(0, H, 2025)
    # the BVH walk returns the linear scan's closest hit for every one of the 335 M segments of this frame
    _assert_frames_equal(full, brute)
    assert np.array_equal(full8, brute8)
    assert 0.2 < np.nanmean(full) < 0.8 and (~np.isfinite(full)).sum() < 30
    # spot-check against the oracle on pixels spread over the frame (100 spp each)
    rng = np.random.default_rng(3)
    for x, y in zip(rng.integers(0, 1200, 24), rng.integers(0, H, 24)):
        want, _ = ob.render_rect_counter(ocam, *rtow, 2025, int(x), int(y), int(x) + 1, int(y) + 1)
        _assert_frames_equal(full[y, x][None, None], want)


def test_config3_full_frame_sharding_invariance(pkg, rtow, gpu):
    """config 3: 1920x1080, 512 spp: the 8-way interleaved row-block render reassembles to the 1-GPU frame."""
    torch = gpu
    cam = pkg.camera_setup(pkg.camera_params(image_width=1920, samples_per_pixel=512, max_depth=50))
    W, H = cam.img_width, cam.img_height
    dev = torch.device("cuda", 0)
    with pkg.Scene(cam, *rtow, device=0) as s:
        full = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        s.render_row_blocks_device(0, H, 1, 1, 2025, full.data_ptr(), 0, torch.cuda.current_stream(dev).cuda_stream)
        plan = pkg.RowShardPlan(H, 8, 8)
        parts = []
        for r in range(8):
            y_first, n_blocks, _ = plan.shard(r)
            rgb = torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev)
            s.render_row_blocks_device(y_first, 8, 8, n_blocks, 2025, rgb.data_ptr(), 0,
                                       torch.cuda.current_stream(dev).cuda_stream)
            parts.append(rgb)
        torch.cuda.synchronize()
        frame = torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev))
        assert torch.equal(frame.view(torch.int32), full.view(torch.int32))
        assert int((~torch.isfinite(full)).sum()) < 30 and 0.2 < float(torch.nanmean(full)) < 0.8


def test_config4_100k_spheres(pkg, ob, gpu):
    """config 4: 100k spheres with a full BVH (2.4 MB of spheres + 6.4 MB of nodes stay in HBM).  The BVH walk, the
    linear scan on the GPU and the oracle's linear scan agree bit for bit."""
    objs, mats, kw = big_grid(316)
    assert len(objs) > 99000
    kw.update(image_width=96, samples_per_pixel=2)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH) as s:
        rgb, rgba = s.render_rows(0, cam.img_height, 31)
        again, _ = s.render_rows(0, cam.img_height, 31)
    assert again.tobytes() == rgb.tobytes()
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BRUTE) as s:
        brute, brute8 = s.render_rows(0, cam.img_height, 31)
    _assert_frames_equal(rgb, brute)
    assert np.array_equal(rgba, brute8)
    rng = np.random.default_rng(5)
    for x, y in zip(rng.integers(0, cam.img_width, 16), rng.integers(0, cam.img_height, 16)):
        want, _ = ob.render_rect_counter(ocam, objs, mats, 31, int(x), int(y), int(x) + 1, int(y) + 1)
        _assert_frames_equal(rgb[y, x][None, None], want)


def test_config5_cornell_full_resolution(pkg, ob, gpu):
    """config 5 shape at full resolution (800x800, 200 bounces; spp cut to 8 to keep the test short): deep-bounce
    paths through both accel paths, and an oracle spot check."""
    objs, mats, kw = cornell_like()
    kw.update(samples_per_pixel=8)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    assert (cam.img_width, cam.img_height, cam.maxdepth) == (800, 800, 200)
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, collect_stats=True) as s:
        rgb, _ = s.render_rows(0, 800, 9)
        st = s.stats()
    assert st["segments"] / st["samples"] > 20  # deep paths indeed
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BRUTE) as s:
        brute, _ = s.render_rows(0, 800, 9)
    _assert_frames_equal(rgb, brute)
    rng = np.random.default_rng(6)
    for x, y in zip(rng.integers(0, 800, 16), rng.integers(0, 800, 16)):
        want, _ = ob.render_rect_counter(ocam, objs, mats, 9, int(x), int(y), int(x) + 1, int(y) + 1)
        _assert_frames_equal(rgb[y, x][None, None], want)


def _bvh_equals_scan(pkg, cam, objs, mats, seed, tunings=(None,)):
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BRUTE) as s:
        want, _ = s.render_rows(0, cam.img_height, seed)
    worst = 0
    for tun in tunings:
        with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, tuning=tun) as s:
            got, _ = s.render_rows(0, cam.img_height, seed)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        worst = max(worst, int((~same).any(axis=-1).sum()))
    return worst


def _decades_world(pkg, seed, m=200):
    """Radii over seven decades, three huge spheres: the regime where the pad's square-root bound matters."""
    rng = np.random.default_rng(seed)
    objs = np.zeros(m, pkg.OBJECT_DTYPE)
    mats = np.zeros(m, pkg.MATERIAL_DTYPE)
    objs["center"] = rng.normal(0.0, 30.0, (m, 3)).astype(np.float32)
    objs["radius"] = (10.0 ** rng.uniform(-3.0, 1.5, m)).astype(np.float32)
    objs["radius"][:3] = (1.0e3, 1.0e4, 3.0e2)
    objs["center"][:3] = ((0.0, -1.0e3, 0.0), (0.0, 0.0, -1.2e4), (350.0, 0.0, 0.0))
    objs["material"] = np.arange(m)
    mats["kind"] = rng.integers(0, 3, m)
    mats["p"] = rng.uniform(0.2, 1.0, (m, 4)).astype(np.float32)
    mats["p"][mats["kind"] == 2, 0] = 1.5
    return objs, mats


def test_bvh_walk_equals_linear_scan_on_generated_worlds(pkg, gpu):
    """The exactness claim of the BVH: for 36 generated worlds -- the reference's generator under other seeds,
    random spheres of mixed radii, jittered grids over an R = 1e4 ground, radii over seven decades seen from 20 to 30 000
    units away -- the walk and the linear scan give bit-identical frames, with the tree in LDS (where the scene fits) and forced
    to stay in HBM -- the same 48-byte node records with fp16 half extents in both layouts, read by walk_nodes_lds and
    walk_nodes_hbm."""
    bad = {}
    for i in range(36):
        if i % 3 == 0:
            objs, mats = pkg.make_world_spheres(1000 + i)
            kw = dict(image_width=400, samples_per_pixel=12, max_depth=50)
        elif i % 3 == 1:
            objs, mats = random_spheres(300 + 40 * i, seed=i, extent=6.0 + i)
            kw = dict(image_width=320, samples_per_pixel=8, max_depth=30)
        elif i % 6 == 2:
            objs, mats, kw = big_grid(24 + 4 * i, seed=i)
            kw.update(image_width=240, samples_per_pixel=4)
        else:
            objs, mats = _decades_world(pkg, i)
            far = (20.0, 2.0e3, 3.0e4)[(i // 6) % 3]
            kw = dict(image_width=240, samples_per_pixel=8, max_depth=40, vertical_fov=50.0, defocus_angle=0.0,
                      focus_distance=10.0, lookfrom=(far, 0.3 * far + 1.0, 0.5 * far), lookat=(0.0, 0.0, 0.0),
                      world_up=(0.0, 1.0, 0.0))
        cam = pkg.camera_setup(pkg.camera_params(**kw))
        # (pad_mode 0: the library's choice -- the refined pad on the wide grids and the decades worlds, the class pad on the
        # S-RTOW worlds; 2 / 1: the other rule forced on the same world)
        # (lds_top_nodes: the staged top of an HBM-resident tree -- all of it that fits by default, none, the first 40 nodes:
        # waves whose lanes read nodes from LDS and from memory in the same trip)
        d = _bvh_equals_scan(pkg, cam, objs, mats, 77 + i, tunings=(dict(kernel=1), dict(force_hbm_scene=1), dict(pad_mode=2),
                                                                     dict(pad_mode=1, force_hbm_scene=1, lds_top_nodes=1),
                                                                     dict(pad_mode=2, force_hbm_scene=1, lds_top_nodes=41)))
        if d:
            bad[i] = d
    assert not bad, bad


def test_bvh_walk_equals_linear_scan_on_grazing_rays(pkg, gpu):
    """Adversarial case for the box pad: every ray of the image grazes a sphere's limb inside the band where the fp32
    discriminant of object.defs.cc:43-50 changes sign (half-width ~25 u max(L, R)^2 / 2R around the silhouette, u = 2^-24),
    seen from 20 to 30 000 units away, for radii from 0.05 to 1000.  A sphere culled by a box that the scan would have
    accepted shows up as a differing pixel."""
    u = 2.0 ** -24
    rng = np.random.default_rng(9)
    objs, mats = _decades_world(pkg, 123, m=64)
    checked = 0
    for target in (3, 7, 11, 0, 2, 19, 33):  # small and huge spheres
        C = objs["center"][target].astype(np.float64)
        R = float(objs["radius"][target])
        for L in (20.0, 1.0e3, 3.0e4):
            if L <= 1.5 * R:
                continue
            view = rng.normal(size=3)
            view /= np.linalg.norm(view)
            O = C + L * view
            side = np.cross(view, (0.0, 1.0, 0.0))
            side /= np.linalg.norm(side)
            limb = C + R * side  # a point of the silhouette as seen from O
            band = 25.0 * u * max(L, R) ** 2 / (2.0 * R)
            span = min(max(16.0 * band, 1e-5 * R), 3.0 * R)  # image height at the limb: +-8 bands around the silhouette
            dist = float(np.linalg.norm(limb - O))
            kw = dict(aspect_ratio=1.0, image_width=96, samples_per_pixel=4, max_depth=4,
                      vertical_fov=float(np.degrees(2.0 * np.arctan(0.5 * span / dist))), defocus_angle=0.0,
                      focus_distance=dist, lookfrom=tuple(float(v) for v in O), lookat=tuple(float(v) for v in limb),
                      world_up=(0.0, 1.0, 0.0))
            cam = pkg.camera_setup(pkg.camera_params(**kw))
            d = _bvh_equals_scan(pkg, cam, objs, mats, 5, tunings=(dict(pad_mode=1), dict(pad_mode=1, force_hbm_scene=1), dict(pad_mode=2),
                                                                   dict(pad_mode=2, force_hbm_scene=1)))
            assert d == 0, (target, R, L, d)
            checked += 1
    assert checked >= 15


def test_config4_full_size(pkg, ob, gpu):
    """BASELINE configs[3] at its own size: 99 857 spheres (scene in HBM), 1920x1080, 256 spp, 50 bounces.  The oracle
    cannot render the frame (its linear scan needs ~0.5 s per PIXEL), so: the frame is reproducible, a row range and an
    8-way interleaved row-block render give the same bits, and 12 pixels equal the oracle's linear scan."""
    torch = gpu
    objs, mats, kw = big_grid(316)
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    W, H = cam.img_width, cam.img_height
    assert (W, H, cam.samples_per_pixel, cam.maxdepth, len(objs)) == (1920, 1080, 256, 50, 316 * 316 + 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH, device=0) as s:
        full = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        s.render_row_blocks_device(0, H, 1, 1, 404, full.data_ptr(), 0, stream)
        again = torch.zeros_like(full)
        s.render_row_blocks_device(0, H, 1, 1, 404, again.data_ptr(), 0, stream)
        part = torch.zeros((37, W, 3), dtype=torch.float32, device=dev)
        s.render_row_blocks_device(611, 37, 1, 1, 404, part.data_ptr(), 0, stream)
        plan = pkg.RowShardPlan(H, 8, 8)
        parts = []
        for r in range(8):
            y_first, n_blocks, _ = plan.shard(r)
            buf = torch.zeros((plan.max_rows, W, 3), dtype=torch.float32, device=dev)
            s.render_row_blocks_device(y_first, 8, 8, n_blocks, 404, buf.data_ptr(), 0, stream)
            parts.append(buf)
        torch.cuda.synchronize()
        frame = torch.cat(parts, 0).index_select(0, torch.as_tensor(plan.index, device=dev))
        bits = lambda t: torch.nan_to_num(t).view(torch.int32)
        assert torch.equal(bits(again), bits(full))
        assert torch.equal(bits(part), bits(full[611:648]))
        assert torch.equal(bits(frame), bits(full))
        host = full.cpu().numpy()
    assert 0.05 < float(np.nanmean(host)) < 0.9
    rng = np.random.default_rng(44)
    for x, y in zip(rng.integers(0, W, 12), rng.integers(H // 3, H, 12)):  # the lower two thirds see the sphere field
        want, _ = ob.render_rect_counter(ocam, objs, mats, 404, int(x), int(y), int(x) + 1, int(y) + 1)
        _assert_frames_equal(host[y, x][None, None], want)


def test_config5_full_size(pkg, ob, gpu):
    """BASELINE configs[4] at its own size: 800x800, 4096 spp, 200 bounces, rendered the way the library and bench.py do by
    default (RTMI_ACCEL_AUTO: the linear scan for a 7-sphere scene, packed attenuation chains multiplied by the resolve pass) and
    with the BVH walk.  The 42 GB of sample records + 210 GB of chain slots exceed the library's buffer cap (a third of the
    device's memory: 96 GB on MI355X), so the call runs in bands of rows without any override (three); both renders give the same
    bits, a row range rendered on its own (one band, straddling a band boundary of the full call) gives the same bits, and 16
    pixels equal the oracle."""
    objs, mats, kw = cornell_like()
    cam, ocam = pkg.camera_setup(pkg.camera_params(**kw)), ob.camera_setup(ob.camera_params(**kw))
    assert (cam.img_width, cam.img_height, cam.samples_per_pixel, cam.maxdepth) == (800, 800, 4096, 200)
    assert 800 * 800 * 4096 * 16 > 24 << 30  # needs the banded path
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_AUTO) as s:  # what bench.py --config 5 times
        li = s.launch_info()
        assert s.accel == pkg.ACCEL_BRUTE and li["packed_chains"] > 0
        rgb, rgba = s.render_rows(0, 800, 55)
        assert s.last_kernel_ms() > 500.0
        assert s.launch_info()["packed_chain_fallbacks"] == 0 and s.launch_info()["whole_pixel_fallbacks"] == 0
        # the full call ran in bands of whole tile rows, as many as the cap (a third of the device's memory) asks for
        n_bands = s.launch_info()["bands"]
        assert 2 <= n_bands <= 12
        band = -(-100 // n_bands) * 8
        part, part8 = s.render_rows(band - 8, band + 8, 55)  # straddles the first band boundary of the full call
    assert rgb[band - 8:band + 8].tobytes() == part.tobytes() and np.array_equal(rgba[band - 8:band + 8], part8)
    with pkg.Scene(cam, objs, mats, accel=pkg.ACCEL_BVH) as s:
        walk, walk8 = s.render_rows(0, 800, 55)
    assert walk.tobytes() == rgb.tobytes() and np.array_equal(walk8, rgba)
    assert np.isfinite(rgb).all() and 0.001 < float(rgb.mean()) < 1.0  # a dark box: light enters through the opening only
    rng = np.random.default_rng(45)
    for x, y in zip(rng.integers(0, 800, 16), rng.integers(0, 800, 16)):
        want, want8 = ob.render_rect_counter(ocam, objs, mats, 55, int(x), int(y), int(x) + 1, int(y) + 1)
        _assert_frames_equal(rgb[y, x][None, None], want)
        assert rgba[y, x] == want8[0, 0]


@pytest.mark.parametrize("config", ["2", "3"])
def test_full_frame_digest_matches_oracle(pkg, rtow, gpu, config):
    """BASELINE configs 2 and 3, WHOLE frame against the oracle's linear scan: the oracle frames took minutes / an hour
    on 8 CPU cores (tests/golden/make_full_frame_hashes.py), so their SHA-256 digests are the fixture.  Equal digests
    mean every float of the frame is bit-identical (NaNs canonicalised)."""
    import hashlib
    path = os.path.join(GOLDEN, "full_frame_hashes.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    if config not in doc:
        pytest.skip("no oracle digest committed for this config")
    ref = doc[config]
    cam = pkg.camera_setup(pkg.camera_params(**ref["camera"]))
    with pkg.Scene(cam, *rtow, accel=pkg.ACCEL_BVH) as s:
        rgb, rgba = s.render_rows(0, cam.img_height, ref["render_seed"])
    u = rgb.view(np.uint32).copy()
    u[np.isnan(rgb)] = 0x7fc00000
    assert int(np.isnan(rgb).any(axis=-1).sum()) == ref["nan_pixels"]
    assert hashlib.sha256(np.ascontiguousarray(rgba).tobytes()).hexdigest() == ref["sha256_rgba8"]
    assert hashlib.sha256(u.tobytes()).hexdigest() == ref["sha256_rgb_float32"]
