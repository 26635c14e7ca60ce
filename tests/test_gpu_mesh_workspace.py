"""-m gpu: the workspaces of the mesh entries - hoisdf_mesh_sdf_rows, hoisdf_eval_interaction, hoisdf_interaction_loss_fwd / _bwd,
hoisdf_eval_surface, hoisdf_iso_extract, hoisdf_raster_meshes - hold exactly what their size queries say.  A query and the carving
of the call it sizes must agree: if the call carved more than the query counted, a kernel would write past the caller's buffer.

Every entry runs twice on the same inputs, straight through the C ABI: once with a workspace of exactly `need` bytes, the first
`need` bytes of one allocation of need + 4096 bytes filled with 0xA5, and once with need + 65536 bytes.  The 4096 bytes behind `need`
must still be 0xA5 afterwards, and every output of the exact call must equal the generous call's bit for bit.

The shapes are the smallest at which the padding between sub-buffers is not zero, so that a dropped round-up to 256 bytes would
move a pointer: B = 3; hand = a cube, 8 vertices, 12 shared faces; object = a tetrahedron, vertex rows padded to V = 5 with a copy
of vertex 0 (obj_n_verts 4, 4, 5), per-sample faces padded to max_faces = 6 with two faces that name the copy and are therefore
degenerate (n_faces 4, 0, 6); n_hand = 5, n_obj = 3; n_samples = 7; an iso grid of 5^3 nodes over a sphere, capacities 64 / 128;
a 16 x 16 image.  The sub-buffers in bytes, in carving order (SIZES below; * = not a multiple of 256, each rounded up to one):
  prepared hand   tris 1728*  area 144*  cdf 144*  box 96*    -> 2560        prepared object  864*  72*  72*  96*  -> 1792
  mesh_sdf_rows   hand, object                                                                                    -> 4352
  interaction     hand, object, sdf_ho 96*, sdf_oh 60*, block counts 3 x 4096 x 4 = 49152                         -> 54016
  loss            hand, object, sdf / face / weights of the hand's vertices 96* 96* 288*, of the object's 60* 60* 180*,
                  denominators 96*                                                                                -> 6400
  eval_surface    object, sdf 96*, samples 252*, squared distances 84*                                            -> 2560
  iso_extract     block vertex counts 12*, block face counts 12*, node words 1500*                                -> 2048
  raster          3 x (12 + 6) records of 64 bytes = 3456*                                                        -> 3584"""
import ctypes as C

import numpy as np
import pytest
import torch

from hoisdf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N_HAND, N_OBJ, N_SAMPLES, ISO_N, ISO_MAX_V, ISO_MAX_F, IMG = 3, 5, 3, 7, 5, 64, 128, 16
VH, FH, VO, FO = 8, 12, 5, 6
CENTRE = np.array([0.03, -0.02, 0.7], np.float32)

CUBE_V = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float32)
CUBE_F = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [0, 4, 7], [0, 7, 3], [1, 2, 6],
                   [1, 6, 5]], np.int32)
TET_V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, 1]], np.float32)        # row 4: a copy of row 0
TET_F = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [0, 4, 1], [4, 0, 2]], np.int32)     # rows 4, 5: degenerate


def _mesh(*faces):
    """tris, area, cdf, box of every prepared mesh"""
    return sum(([B * f * 48, B * f * 4, B * f * 4, B * 32] for f in faces), [])


SIZES = {
    "hoisdf_mesh_sdf_rows_workspace_bytes": ((B, FH, FO), _mesh(FH, FO)),
    "hoisdf_eval_interaction_workspace_bytes": ((B, VH, FH, VO, FO), _mesh(FH, FO) + [B * VH * 4, B * VO * 4, B * (64 ** 3 // 64) * 4]),
    "hoisdf_interaction_loss_workspace_bytes": ((B, VH, FH, VO, FO), _mesh(FH, FO) + [B * VH * 4, B * VH * 4, B * VH * 12, B * VO * 4,
                                                                                      B * VO * 4, B * VO * 12, B * 32]),
    "hoisdf_eval_surface_workspace_bytes": ((B, VH, FO, N_SAMPLES), _mesh(FO) + [B * VH * 4, B * N_SAMPLES * 12, B * N_SAMPLES * 4]),
    "hoisdf_iso_extract_workspace_bytes": ((B, ISO_N), [B * 1 * 4, B * 1 * 4, B * ISO_N ** 3 * 4]),       # 125 nodes: one block of 256
    "hoisdf_raster_workspace_bytes": ((B, FH, FO), [B * (FH + FO) * 64]),
}
NEED = {"hoisdf_mesh_sdf_rows_workspace_bytes": 4352, "hoisdf_eval_interaction_workspace_bytes": 54016,
        "hoisdf_interaction_loss_workspace_bytes": 6400, "hoisdf_eval_surface_workspace_bytes": 2560,
        "hoisdf_iso_extract_workspace_bytes": 2048, "hoisdf_raster_workspace_bytes": 3584}


def need(query):
    """the size the library states, held to the formula evaluated here: every sub-buffer rounded up to 256 bytes"""
    dims, parts = SIZES[query]
    n = getattr(_lib.lib(), query)(*dims)
    assert n == sum((s + 255) // 256 * 256 for s in parts) == NEED[query], (query, n, parts)
    assert any(s % 256 for s in parts), (query, "no padding between the sub-buffers: a dropped round-up would not show")
    return n


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


_IN = {}


def inputs():
    """the device arrays every case reads and the two descriptors over them: made once, never written"""
    if not _IN:
        assert _lib.CONSTANTS["INTERACT_MAX_GRID"] == 64 and _lib.CONSTANTS["MESH_MAX_FACES"] >= FH
        r = np.random.default_rng(3)
        jit = lambda v: (v + r.normal(0, 0.0002, v.shape)).astype(np.float32)
        hv = np.stack([jit(CUBE_V * 0.02 + CENTRE) for _ in range(B)])
        ov = np.stack([jit(TET_V[:4] * 0.015 + CENTRE + np.float32([0.015, 0.005, 0.0])) for _ in range(B)])
        ov = np.concatenate([ov, ov[:, :1]], 1)                                                      # the padding row: vertex 0 again
        t = dict(hv=gpu(hv), hf=gpu(CUBE_F), ov=gpu(ov), of=gpu(np.stack([TET_F] * B)), on=gpu(np.int32([4, 0, 6])),
                 onv=gpu(np.int32([4, 4, 5])), lab=gpu(np.arange(VH, dtype=np.int32) % 6), pn=gpu(np.int32([8, 5, 0])),
                 g=gpu(np.float32([[0.7, 1.3, 0.9], [1.1, 0.6, 1.4], [0.8, 1.2, 0.5]]).T))
        assert t["hv"].shape == (B, VH, 3) and t["hf"].shape == (FH, 3) and t["ov"].shape == (B, VO, 3) and t["of"].shape == (B, FO, 3)
        t["hand"] = _lib.Mesh(verts=t["hv"].data_ptr(), faces=t["hf"].data_ptr(), n_faces=None, face_batch_stride=0, V=VH, max_faces=FH)
        t["obj"] = _lib.Mesh(verts=t["ov"].data_ptr(), faces=t["of"].data_ptr(), n_faces=t["on"].data_ptr(), face_batch_stride=3 * FO,
                             V=VO, max_faces=FO)
        # a sphere of 6 mm around the middle node of 5^3 nodes 10 mm apart: one node inside, 14 vertices
        ax = np.arange(ISO_N, dtype=np.float32) * 0.01
        x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
        d = np.sqrt((x - 0.02) ** 2 + (y - 0.02) ** 2 + (z - 0.02) ** 2) - 0.006
        t["values"] = gpu(np.stack([d.reshape(-1)] * B).astype(np.float32))      # symmetric: the same field in either node order
        t["grid"] = gpu(np.float32([[0, 0, 0, 0.01, 0.01, 0.01, 0, 0]] * B))
        t["K"] = gpu(np.float32([[120, 0, 3, 0, 120, 11]] * B))                                      # both meshes inside the 16 x 16 image
        _IN.update(t)
    return _IN


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, device=DEV, dtype=dtype)


def exact_and_generous(query, run):
    """run(workspace tensor, bytes to state) -> dict of the call's outputs (zeroed tensors of its own); the two assertions"""
    n = need(query)
    guarded = torch.full((n + 4096,), 0xA5, device=DEV, dtype=torch.uint8)
    exact = run(guarded, n)
    generous = run(torch.full((n + 65536,), 0xA5, device=DEV, dtype=torch.uint8), n + 65536)
    torch.cuda.synchronize()
    tail = guarded[n:].cpu().numpy()
    assert (tail == 0xA5).all(), (query, "bytes written behind the workspace, the first at", n + int(np.flatnonzero(tail != 0xA5)[0]))
    assert exact.keys() == generous.keys() and len(exact) > 0
    for k in exact:
        a, b = exact[k].cpu().numpy(), generous[k].cpu().numpy()
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (query, k)
    return exact


def test_mesh_sdf_rows():
    t = inputs()

    def run(ws, nws):
        rows = zeros(B, N_HAND + N_OBJ, 6)
        _lib.call("hoisdf_mesh_sdf_rows", C.addressof(t["hand"]), C.addressof(t["obj"]), p(t["lab"]), B, N_HAND, N_OBJ, 0.01, 0.003, 4, 0.05,
                  0.05, 11, p(rows), 6, p(ws), nws, st())
        return {"rows": rows}

    rows = exact_and_generous("hoisdf_mesh_sdf_rows_workspace_bytes", run)["rows"].cpu().numpy()
    assert np.isfinite(rows[:, :, :4]).all() and (np.abs(rows[:, :, 3]) < 0.2).all(), "the call did run: distances to the hand"


def test_eval_interaction():
    t = inputs()

    def run(ws, nws):
        o = {k: zeros(B) for k in ("pen_hand", "pen_obj", "min_dist", "volume")}
        o.update({k: zeros(B, dtype=torch.int32) for k in ("contact_verts", "in_contact", "inside_count")})
        o["inside"], o["grid"] = zeros(B, 64 ** 3, dtype=torch.uint8), zeros(B, 8)
        _lib.call("hoisdf_eval_interaction", C.addressof(t["hand"]), C.addressof(t["obj"]), p(t["onv"]), B, 0.005, 0.005, p(o["pen_hand"]),
                  p(o["pen_obj"]), p(o["min_dist"]), p(o["contact_verts"]), p(o["in_contact"]), p(o["volume"]), p(o["inside_count"]),
                  p(o["inside"]), p(o["grid"]), p(ws), nws, st())
        return o

    o = exact_and_generous("hoisdf_eval_interaction_workspace_bytes", run)
    count = o["inside_count"].cpu().numpy()
    assert count[0] > 0 and count[2] > 0 and count[1] == 0, "the meshes overlap where the object has faces"


def test_interaction_loss_fwd_then_bwd():
    t = inputs()

    def run(ws, nws):
        o = {k: zeros(B) for k in ("rep_hand", "att", "rep_obj")}
        o["d_hand"], o["d_obj"] = zeros(B, VH, 3), zeros(B, VO, 3)
        head = (C.addressof(t["hand"]), C.addressof(t["obj"]), p(t["onv"]), B, None, 0, None, 0, None, 0, 0.01)
        _lib.call("hoisdf_interaction_loss_fwd", *head, p(o["rep_hand"]), p(o["att"]), p(o["rep_obj"]), p(ws), nws, st())
        g = t["g"]
        _lib.call("hoisdf_interaction_loss_bwd", *head, p(g[0]), p(g[1]), p(g[2]), p(o["d_hand"]), p(o["d_obj"]), p(ws), nws, st())
        return o

    o = exact_and_generous("hoisdf_interaction_loss_workspace_bytes", run)
    assert float(o["att"][0]) > 0 and float(o["rep_obj"][0]) > 0 and float(o["d_hand"][0].abs().max()) > 0, "the backward read what the forward left"


def test_eval_surface():
    t = inputs()

    def run(ws, nws):
        o = {k: zeros(B) for k in ("pred_to_gt", "gt_to_pred", "chamfer")}
        o["n_used"], o["nearest"] = zeros(B, dtype=torch.int32), zeros(B, N_SAMPLES, dtype=torch.int32)
        _lib.call("hoisdf_eval_surface", p(t["hv"]), p(t["pn"]), VH, C.addressof(t["obj"]), B, N_SAMPLES, 5, p(o["pred_to_gt"]),
                  p(o["gt_to_pred"]), p(o["chamfer"]), p(o["n_used"]), None, p(o["nearest"]), p(ws), nws, st())
        return o

    o = exact_and_generous("hoisdf_eval_surface_workspace_bytes", run)
    assert o["n_used"].tolist() == [8, 0, 0] and float(o["chamfer"][0]) > 0, "sample 1 has no face, sample 2 no predicted vertex"


def test_iso_extract():
    t = inputs()

    def run(ws, nws):
        o = {"verts": zeros(B, ISO_MAX_V, 3), "faces": zeros(B, ISO_MAX_F, 3, dtype=torch.int32), "n_verts": zeros(B, dtype=torch.int32),
             "n_faces": zeros(B, dtype=torch.int32)}
        _lib.call("hoisdf_iso_extract", p(t["values"]), 1, p(t["grid"]), ISO_N, B, 0.0, 1.0, None, p(o["verts"]), ISO_MAX_V, p(o["faces"]),
                  ISO_MAX_F, p(o["n_verts"]), p(o["n_faces"]), p(ws), nws, st())
        return o

    o = exact_and_generous("hoisdf_iso_extract_workspace_bytes", run)
    nv, nf = o["n_verts"].tolist(), o["n_faces"].tolist()
    assert 0 < nv[0] <= ISO_MAX_V and 0 < nf[0] <= ISO_MAX_F and nv == [nv[0]] * B and nf == [nf[0]] * B, (nv, nf)


def test_raster_meshes():
    t = inputs()

    def run(ws, nws):
        o = {"ids": zeros(B, IMG, IMG, dtype=torch.int32), "depth": zeros(B, IMG, IMG), "hand_seg": zeros(B, 8, 8), "obj_seg": zeros(B, 8, 8),
             "counts": zeros(B, 2, dtype=torch.int32)}
        _lib.call("hoisdf_raster_meshes", C.addressof(t["hand"]), C.addressof(t["obj"]), p(t["K"]), B, IMG, IMG, 0, 0.01, p(o["ids"]),
                  p(o["depth"]), p(o["hand_seg"]), p(o["obj_seg"]), 8, 8, p(o["counts"]), p(ws), nws, st())
        return o

    o = exact_and_generous("hoisdf_raster_workspace_bytes", run)
    counts = o["counts"].cpu().numpy()
    assert (counts[:, 0] > 0).all() and counts[0, 1] > 0 and counts[1, 1] == 0, counts
