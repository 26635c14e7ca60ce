"""CPU: hoisdf_amd/raster_oracle.py, the numpy restatement of the raster rules of include/hoisdf.h, against closed forms and against
an independent float64 ray caster: coverage partitions shared edges and vertices, depth is perspective-correct, ids and masks are
those of the ray cast away from the edges, and the tie, skip and fold rules are the header's."""
import numpy as np
import pytest

from hoisdf_amd import raster_oracle as ro

TRI = np.float32([[-0.2, -0.2, 1], [0.25, -0.15, 1], [-0.1, 0.25, 1]])
F1 = np.int32([[0, 1, 2]])
K48 = np.float32([64, 0, 24, 0, 64, 24])


@pytest.mark.parametrize("half", (0, 1))
def test_a_split_quad_partitions_its_pixels(half):
    v, f, K, W, H = ro.quad_case()
    ids, depth, cover, counts = ro.raster([(v, f), None], K, W, H, half)
    want = np.zeros((H, W), np.int32)
    want[8:40, 8:40] = 1
    assert np.array_equal(cover, want), "exactly once on [8, 40) x [8, 40): the left and top edges in, the right and bottom out"
    assert np.bincount(ids[ids >= 0]).tolist() == [528, 496], "the diagonal's pixels belong to one face"
    assert counts.tolist() == [1024, 0] and (depth[ids >= 0] == 1).all() and (depth[ids < 0] == 0).all()
    # the same quad wound the other way and with the other diagonal
    ids2, _, cover2, _ = ro.raster([None, (v, np.int32([[1, 0, 3], [1, 3, 2]]))], K, W, H, half)
    assert np.array_equal(cover2, want) and (ids2[ids2 >= 0] >> 16 == 1).all()


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("n", (6, 7, 12))
def test_a_fan_gives_its_centre_to_exactly_one_face(n, half):
    v, f, K, W, H = ro.fan_case(n)
    ids, _, cover, counts = ro.raster([(v, f), None], K, W, H, half)
    assert cover.max() == 1 and counts[0] == cover.sum() > 600
    if not half:
        assert cover[24, 24] == 1, "the shared vertex sits on this sample point"
    # every pixel well inside the rim polygon is covered
    yy, xx = np.mgrid[0:H, 0:W] + (0.5 if half else 0.0)
    assert (cover[np.hypot(xx - 24, yy - 24) < 15.5 * np.cos(np.pi / n) - 0.01] == 1).all()


def test_depth_is_perspective_correct():
    v, f, K, W, H, zt = ro.plane_case()
    ids, depth, cover, _ = ro.raster([(v, f), None], K, W, H, 1)
    assert (cover == 1).all() and (ids >= 0).all()
    ulp = np.spacing(zt.astype(np.float32)).astype(np.float64)[:, None]
    err = np.abs(depth.astype(np.float64) - zt[:, None]) / ulp
    print("depth error in float32 ulps:", err.max())
    assert err.max() <= 1.0
    linear = 1 + (np.arange(64) + 0.5) / 64                                  # what interpolating z in screen space would give
    assert np.abs(linear - zt).max() > 0.15 and np.abs(depth[:, 0] - linear).max() > 0.15


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("size", ((64, 64, 300.0), (96, 64, 420.0)))
def test_ids_and_masks_equal_a_float64_ray_cast_away_from_the_edges(size, half):
    """Snapping to 1/256 pixel moves a projected edge by at most sqrt(2)/512 pixel, so a sample point at least 1/256 pixel from
    every projected edge is on the same side of every edge in both pictures: there the two must agree without exception"""
    W, H, fx = size
    meshes, K = ro.sphere_torus_case(W, H, fx)
    ids, depth, _, counts = ro.raster(meshes, K, W, H, half)
    cid, cz, near_edge = ro.raycast(meshes, K, W, H, half)
    covered = (ids >= 0) | (cid >= 0)
    band = (near_edge & covered).sum() / covered.sum()
    print(f"{W} x {H} half_pixel {half}: {covered.sum()} covered, hand {counts[0]}, object {counts[1]}, left out {100 * band:.2f} %")
    assert covered.sum() > 3000 and counts.min() > 500
    assert band <= 0.03
    ok = ~near_edge
    assert ((ids != cid) & ok).sum() == 0
    for m in (0, 1):
        assert np.array_equal(((ids >= 0) & (ids >> 16 == m))[ok], ((cid >= 0) & (cid >> 16 == m))[ok])


def test_exact_depth_ties():
    ids, _, _, counts = ro.raster([(TRI, F1), (TRI, F1)], K48, 48, 48)
    assert counts[0] > 100 and counts[1] == 0, "the hand wins over the object"
    v6 = np.concatenate([TRI, TRI])
    ids, _, cover, counts = ro.raster([None, (v6, np.int32([[3, 4, 5], [0, 1, 2], [0, 2, 1]]))], K48, 48, 48)
    assert (ids[ids >= 0] == 1 << 16).all() and cover.max() == 3, "the lower face row wins within a mesh"
    # a nearer object still wins over the hand
    ids, _, _, counts = ro.raster([(TRI, F1), (TRI * np.float32(0.5), F1)], K48, 48, 48)
    assert counts[1] > 100 and counts[0] == 0


@pytest.mark.parametrize("name, verts, faces, near", (
    ("behind_near", TRI * np.float32([1, 1, 0.5]), F1, 0.75),
    ("crossing_near", np.float32([[-0.2, -0.2, 0.7], [0.25, -0.15, 1], [-0.1, 0.25, 1]]), F1, 0.75),
    ("a_nan_corner", np.float32([[-0.2, np.nan, 1], [0.25, -0.15, 1], [-0.1, 0.25, 1]]), F1, 0.01),
    ("an_inf_corner", np.float32([[-0.2, -0.2, np.inf], [0.25, -0.15, 1], [-0.1, 0.25, 1]]), F1, 0.01),
    ("the_guard_band", np.float32([[-0.2, -0.2, 1], [300.0, -0.15, 1], [-0.1, 0.25, 1]]), F1, 0.01),
    ("zero_snapped_area", np.float32([[0, 0, 1], [1e-5, 0, 1], [0, 1e-5, 1]]), F1, 0.01),
    ("a_repeated_vertex", TRI, np.int32([[0, 1, 1]]), 0.01),
    ("an_index_too_large", TRI, np.int32([[0, 1, 3]]), 0.01),
    ("a_negative_index", TRI, np.int32([[0, -1, 2]]), 0.01)))
def test_each_skip_rule(name, verts, faces, near):
    ids, depth, cover, counts = ro.raster([(verts, faces), (TRI, F1)], K48, 48, 48, 0, near)
    assert counts[0] == 0 and cover.max() == 1, "the hand's face takes no part"
    alone = ro.raster([None, (TRI, F1)], K48, 48, 48, 0, near)
    assert np.array_equal(ids, alone[0]) and np.array_equal(depth, alone[1]) and counts[1] == alone[3][1] > 100
    # the face beside a skipped one is drawn, and keeps its row as its id
    ids, _, _, counts = ro.raster([(np.concatenate([verts, TRI]), np.concatenate([faces, F1 + 3])), None], K48, 48, 48, 0, near)
    assert counts[0] == alone[3][1] and (ids[ids >= 0] == 1).all()


def test_the_guard_band_is_where_the_header_puts_it():
    at = lambda x: ro.raster([(np.float32([[-0.2, -0.2, 1], [x, -0.15, 1], [-0.1, 0.25, 1]]), F1), None], K48, 48, 48)[3][0]
    assert at((16383.9 - 24) / 64) > 0 and at((16384.0 - 24) / 64) == 0 and at(-(16384.0 + 24) / 64) == 0


def test_faces_partly_and_wholly_off_screen():
    big = np.float32([[-3, -3, 1], [4, -2, 1], [-1, 5, 1]])
    ids, _, cover, counts = ro.raster([(big, F1), None], K48, 48, 48)
    wide = ro.raster([(big, F1), None], K48 + np.float32([0, 0, 256, 0, 0, 256]), 560, 560)
    assert np.array_equal(cover, wide[2][256:304, 256:304]), "the image is a window of a larger one"
    assert 0 < counts[0] == cover.sum()
    for shift in ([5, 0, 0], [0, -5, 0], [-5, 5, 0]):
        ids, depth, cover, counts = ro.raster([(TRI + np.float32(shift), F1), None], K48, 48, 48)
        assert (ids == -1).all() and (depth == 0).all() and not cover.any() and counts.tolist() == [0, 0]


def test_an_empty_mesh_and_a_missing_one():
    empty = (TRI, np.zeros((0, 3), np.int32))
    a = ro.raster([empty, (TRI, F1)], K48, 48, 48)
    b = ro.raster([None, (TRI, F1)], K48, 48, 48)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[3][1] > 100
    c = ro.raster([empty, None], K48, 48, 48)
    assert (c[0] == -1).all() and c[3].tolist() == [0, 0]


@pytest.mark.parametrize("fx, fy", ((2, 2), (4, 4), (2, 4), (4, 2), (1, 1)))
def test_fold_masks_reads_the_pixel_image_crop_reads(fx, fy):
    rng = np.random.default_rng(3)
    W, H = 24, 16
    ids = rng.integers(-1, 2, (2, H, W)).astype(np.int32)
    ids = np.where(ids > 0, 1 << 16 | 5, ids)                                 # -1, hand face 0, object face 5
    hand, obj = ro.fold_masks(ids, W // fx, H // fy)
    assert hand.shape == obj.shape == (2, H // fy, W // fx) and hand.dtype == np.float32
    for j in range(H // fy):
        for i in range(W // fx):
            src = ids[:, int((j + 0.5) * fy), int((i + 0.5) * fx)]          # floor((i + .5) res / hm) per axis, as hoisdf_image_crop
            assert np.array_equal(hand[:, j, i], (src == 0).astype(np.float32)) and np.array_equal(obj[:, j, i], (src > 0).astype(np.float32))
    with pytest.raises(ValueError):
        ro.fold_masks(ids, 5, 4)


def test_overlay_and_silhouette_counts_by_hand():
    ids = np.int32([[-1, 0, 7], [1 << 16, 1 << 16 | 9, -1]])
    img = np.uint8([[[10, 20, 30], [10, 20, 30], [255, 0, 128]], [[0, 0, 0], [255, 255, 255], [1, 2, 3]]])
    col = ((200, 100, 0), (0, 50, 255))
    out = ro.overlay(ids, img, col, 128)
    assert out.tolist() == [[[10, 20, 30], [105, 60, 15], [228, 50, 64]], [[0, 25, 128], [128, 153, 255], [1, 2, 3]]]
    assert np.array_equal(ro.overlay(ids, img, col, 0), img)
    assert ro.overlay(ids, img, col, 256)[0, 1].tolist() == [200, 100, 0] and ro.overlay(ids, img, col, 256)[1, 0].tolist() == [0, 50, 255]
    ph = np.float32([[1, 1, 0, 0, 0.5], [0, 0, 0, 0, 0]])
    gh = np.float32([[1, 0, 1, 0, 0.6], [0, 0, 0, 0, 0]])
    po = np.float32([[0, 0, 0, 0, 1], [1, 1, 1, 0, 0]])
    go = np.float32([[0, 0, 0, 0, 1], [1, 1, 1, 0, 0.51]])
    assert ro.silhouette_counts(ph, po, gh, go).tolist() == [[1, 4, 1, 1], [0, 0, 3, 4]]
