"""-m gpu: the evaluation metrics as HIP kernels (csrc/eval.hip; hoisdf_eval_*, ops.eval_*, metrics.*_native, metrics.Evaluator) against
  - g11_metrics.npz = the REFERENCE's own metric functions, at the bars tests/test_metrics_golden.py holds the torch path to;
  - an fp64 numpy restatement written here, on the shapes where tiles and reductions can go wrong;
  - exact threshold counts where fp64 says no distance is near a threshold;
  - themselves: pieces against one feed, two calls, the torch Evaluator, a plain C host.
Bars (all absolute, metres or ratios), from tests/test_metrics_golden.py: MJE 1e-7, PA-MJE 1e-6, aligned points 1e-5, ADDS / MCE / OCE /
MME 2e-6, F-scores 1e-6, mesh mean 1e-8, AUC and PCK 1e-6.  Seeds are chosen on the CPU from the fp64 restatement alone (the conditions
they meet are asserted, over every sample); nothing here depends on what the kernels return."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden
from hoisdf_amd import metrics as M
from hoisdf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = dict(mje=1e-7, pamje=1e-6, aligned=1e-5, obj=2e-6, fscore=1e-6, mesh_mean=1e-8, auc=1e-6, pck=1e-6, xform=1e-5)
F_TH = [0.005, 0.015]
# fp32 distances carry up to ~2 ulp (1.2e-7 relative) of rounding: a count can differ from the fp64 count only for a distance this
# close to a threshold.  The shape cases below assert that fp64 sees none within NEAR; the exact-count test asks the issue's 1e-5.
NEAR = 4e-7


def held(name, value, bar):
    print(f"{name}: {value:.3e} (bar {bar:.0e})")
    assert value < bar, f"{name}: {value:.3e} >= {bar:.0e}"


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


# ---- the fp64 restatement (numpy, CPU) -------------------------------------------------------------------------------------------
def np_rodrigues(aa):
    """metrics.batch_rodrigues in fp64: (B,3) -> (B,3,3)"""
    aa = np.asarray(aa, np.float64)
    ang = np.linalg.norm(aa + 1e-8, axis=1, keepdims=True)
    q = np.concatenate([np.cos(0.5 * ang), np.sin(0.5 * ang) * aa / ang], 1)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                  2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                  2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1)
    return R.reshape(-1, 3, 3)


def np_nn(q, s):
    """distance of every point of q (n,3) to its nearest point of s (m,3), fp64, differences squared directly"""
    q, s = np.asarray(q, np.float64), np.asarray(s, np.float64)
    d2 = np.zeros((len(q), len(s)))
    for c in range(3):
        d2 += (q[:, None, c] - s[None, :, c]) ** 2
    return np.sqrt(d2.min(1))


_CORNERS = np.array([[0, 1, 0, 0, 1, 0, 1, 1], [0, 0, 1, 0, 1, 1, 0, 1], [0, 0, 0, 1, 0, 1, 1, 1]])


def np_object(obj_rot, obj_trans, rot_gt, trans_gt, templates, ids):
    """common/metrics.py:62-185 per sample in fp64 -> dict of (B,) arrays; a negative id: zeros, used = 0"""
    B = len(ids)
    out = {k: np.zeros(B) for k in ("adds", "mce", "oce", "mme")}
    out["used"] = np.zeros(B, np.int32)
    rot, trans = np.asarray(obj_rot, np.float64).mean(1), np.asarray(obj_trans, np.float64).mean(1)
    Rp, Rg = np_rodrigues(rot), np_rodrigues(rot_gt)
    for b in range(B):
        if ids[b] < 0:
            continue
        tpl = np.asarray(templates[ids[b]], np.float64)
        prd, tgt = tpl @ Rp[b].T + trans[b], tpl @ Rg[b].T + np.asarray(trans_gt[b], np.float64)
        out["adds"][b] = np_nn(prd, tgt).mean()
        mm_p, mm_t = np.stack([prd.min(0), prd.max(0)], 1), np.stack([tgt.min(0), tgt.max(0)], 1)      # (3,2)
        cp = np.stack([mm_p[0, _CORNERS[0]], mm_p[1, _CORNERS[1]], mm_p[2, _CORNERS[2]]], 1)
        ct = np.stack([mm_t[0, _CORNERS[0]], mm_t[1, _CORNERS[1]], mm_t[2, _CORNERS[2]]], 1)
        out["mce"][b] = np.linalg.norm(cp - ct, axis=1).mean()
        out["oce"][b] = np.linalg.norm(trans[b] - np.asarray(trans_gt[b], np.float64))
        out["mme"][b] = np.linalg.norm(tgt - prd, axis=1).mean()
        out["used"][b] = 1
    return out


def np_procrustes(A, B):
    """common/metrics.py:188-210 on one sample in fp64 -> c, R, t, aligned, singular values of H, reflection branch taken"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb) / len(A)
    U, s, Vt = np.linalg.svd(H)
    sv = s.copy()
    R = Vt.T @ U.T
    neg = np.linalg.det(R) < 0
    if neg:
        s[-1] = -s[-1]
        Vt[2] = -Vt[2]
        R = Vt.T @ U.T
    c = s.sum() / A.var(0).sum()
    t = cb - c * R @ ca
    return c, R, t, (c * R @ A.T).T + t, sv, neg


def np_fscore(d_gt, d_pr, th):
    """eval_util.py:117-136 from nearest distances: gt -> pred (precision), pred -> gt (recall)"""
    p, r = (d_gt < th).mean(), (d_pr < th).mean()
    return 2 * p * r / (p + r) if p + r > 0 else 0.0


def np_measures(dist, th):
    """EvalUtil.get_measures for fully visible meshes: dist (N,V) -> mean EPE, AUC, PCK curve"""
    trapz = getattr(np, "trapezoid", None) or np.trapz
    pck = (dist[None] <= th[:, None, None]).mean(1)
    return dist.mean(0).mean(), (trapz(pck, th, axis=0) / trapz(np.ones_like(th), th)).mean(), pck.mean(1)


def rel_gap(d, ths):
    """smallest |d - th| / th over all distances and all positive thresholds"""
    d = np.asarray(d, np.float64).reshape(-1)
    return min(float(np.abs(d - t).min() / t) for t in ths if t > 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_object(B, V, P, seed, T=5):
    r = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)
    ids = r.integers(0, T, B).astype(np.int32)                    # repeated and out of order
    if B > 8:
        ids[7] = -1                                               # one sample that is not evaluated
        ids[8], ids[9] = ids[6], T - 1
    return dict(templates=f(0.05 * r.standard_normal((T, V, 3))), obj_rot=f(0.3 * r.standard_normal((B, P, 3))),
                obj_trans=f(0.05 * r.standard_normal((B, P, 3))), rot_gt=f(0.3 * r.standard_normal((B, 3))),
                trans_gt=f(0.05 * r.standard_normal((B, 3))), ids=ids)


def make_mesh(B, V, seed):
    r = np.random.default_rng(seed)
    gt = np.asarray(0.05 * r.standard_normal((B, V, 3)), np.float32)
    pr = np.asarray(1.05 * gt + 0.004 * r.standard_normal((B, V, 3)) + 0.003, np.float32)
    return gt, pr


def mesh_reference(gt, pr, acc_th):
    """everything hoisdf_eval_mesh + the accumulators produce, in fp64"""
    B, V = gt.shape[:2]
    ref = dict(d_raw=np.linalg.norm(gt.astype(np.float64) - pr, axis=2))
    if V >= 3:
        ref["aligned"] = np.stack([np_procrustes(pr[b], gt[b])[3] for b in range(B)])
        al32 = ref["aligned"].astype(np.float32).astype(np.float64)           # the aligned points are fp32 values: distances start from those
        ref["d_al"] = np.linalg.norm(gt.astype(np.float64) - al32, axis=2)
    nn = {"raw": [(np_nn(gt[b], pr[b]), np_nn(pr[b], gt[b])) for b in range(B)]}
    if V >= 3:
        nn["al"] = [(np_nn(gt[b], al32[b]), np_nn(al32[b], gt[b])) for b in range(B)]
    ref["nn"] = nn
    for k, key in (("raw", "fs"), ("al", "fs_al")):
        if k in nn:
            ref[key] = np.array([[np_fscore(a, b_, t) for t in F_TH] for a, b_ in nn[k]])
    ref["acc_th"] = acc_th
    ref["measures"] = np_measures(ref["d_raw"], acc_th)
    if V >= 3:
        ref["measures_al"] = np_measures(ref["d_al"], acc_th)
    return ref


def mesh_gaps(ref):
    """(smallest relative gap of a nearest distance to an F-score threshold, of a vertex distance to a PCK threshold)"""
    nn = np.concatenate([np.concatenate(pair) for k in ref["nn"] for pair in ref["nn"][k]])
    d = np.concatenate([ref[k].reshape(-1) for k in ("d_raw", "d_al") if k in ref])
    return rel_gap(nn, F_TH), rel_gap(d, ref["acc_th"])


# (V, B, P, seed): every V, B and P of the issue; a seed is kept if fp64 sees no distance within NEAR of a threshold (checked on the CPU:
# 0 does for every case; the exact-count test needs 1 for its wider 1e-5)
CASES = [(1, 33, 1, 0), (50, 1, 40, 0), (300, 33, 200, 0), (778, 1, 1, 0), (1000, 33, 40, 0), (2049, 1, 200, 0)]
ACC_TH = np.linspace(0.0, 0.05, 20)


# ---- 1. the reference's fixture ----------------------------------------------------------------------------------------------------
def test_reference_fixture(tmp_path):
    g = load_golden("g11_metrics")
    t = lambda k: (g[k] if torch.is_tensor(g[k]) else torch.from_numpy(np.asarray(g[k]))).to(DEV)
    mje, pamje = M.eval_hand_joint_native(t("pred_j"), t("gt_j"))
    held("MJE", abs(mje - float(g["mje"])), BAR["mje"])
    held("PA-MJE", abs(pamje - float(g["pamje"])), BAR["pamje"])
    held("aligned joints", (M.rigid_align_native(t("pred_j"), t("gt_j")).cpu().double() - torch.as_tensor(g["aligned"])).abs().max().item(),
         BAR["aligned"])
    ids = torch.from_numpy(np.asarray(g["obj_cls"])).long() - 1
    args = (t("obj_rot"), t("obj_trans"), t("obj_rot_gt"), t("obj_trans_gt"), t("templates"), ids)
    o = M.obj_metrics_native(*args, ho3d=False)                                    # the dexycb form
    assert set(o) == {"ADDS", "MCE", "OCE"}
    for k, ref in (("ADDS", "adds"), ("MCE", "mce"), ("OCE", "oce")):
        held(f"dexycb {k}", abs(o[k] - float(g[ref])), BAR["obj"])
    o = M.obj_metrics_native(*args, ho3d=True)                                     # the ho3d form
    assert set(o) == {"ADDS", "MME"}
    held("ho3d ADDS", abs(o["ADDS"] - float(g["adds_ho3d"])), BAR["obj"])
    held("ho3d MME", abs(o["MME"] - float(g["mme_ho3d"])), BAR["obj"])
    gt_v, pr_v = t("gt_v"), t("pr_v")
    fs = torch.stack([M.fscore_native(gt_v, pr_v, th) for th in F_TH], 1).cpu().numpy()
    held("F-scores", np.abs(fs - np.asarray(g["fscore_bruteforce"])).max(), BAR["fscore"])
    d0, _, f0, _, _ = ops.eval_mesh(pr_v, gt_v, F_TH)
    held("F-scores (one call)", np.abs(f0.cpu().numpy() - np.asarray(g["fscore_bruteforce"])).max(), BAR["fscore"])
    ev, ev2 = M.MeshEvalNative(), M.MeshEvalNative()
    ev.feed(gt_v[:3], pr_v[:3])                                                    # 3 + 3, as the torch test feeds it
    ev.feed(gt_v[3:], pr_v[3:])
    ev2.feed_dist(d0[:3])
    ev2.feed_dist(d0[3:])
    for e in (ev, ev2):
        m3d, med, auc, pck, th = e.get_measures(0.0, 0.05, 100)
        assert np.isnan(med) and len(pck) == 100 and np.array_equal(th, np.linspace(0.0, 0.05, 100))
        held("mesh mean", abs(m3d - float(g["mesh_mean"])), BAR["mesh_mean"])
        held("mesh AUC", abs(auc - float(g["mesh_auc"])), BAR["auc"])
        held("mesh PCK", np.abs(pck - np.asarray(g["mesh_pck"])).max(), BAR["pck"])
    p = os.path.join(tmp_path, "results.txt")                                      # the writer takes the native accumulators as they are
    M.write_results(p, {"ADDS_error": 12.0}, 6, mesh=(ev, ev2), fscores=(fs.T, fs.T, F_TH))
    lines = open(p).read().splitlines()
    assert lines[1] == "Evaluation 3D MESH results:" and lines[2].startswith("auc=0.809, mean_vert3d_avg=0.96 cm")


# ---- 2. the fp64 restatement on the shapes where tiles and reductions can go wrong ---------------------------------------------
@pytest.mark.parametrize("V,B,P,seed", CASES)
def test_object_metrics_against_fp64(V, B, P, seed):
    x = make_object(B, V, P, seed)
    ref = np_object(x["obj_rot"], x["obj_trans"], x["rot_gt"], x["trans_gt"], x["templates"], x["ids"])
    adds, mce, oce, mme, used = ops.eval_object(dev(x["obj_rot"]), dev(x["obj_trans"]), dev(x["rot_gt"]), dev(x["trans_gt"]),
                                                dev(x["templates"]), torch.from_numpy(x["ids"]))
    got = dict(adds=adds, mce=mce, oce=oce, mme=mme)
    assert np.array_equal(used.cpu().numpy(), ref["used"])
    for k in ("adds", "mce", "oce", "mme"):
        held(f"V={V} B={B} P={P} {k}", np.abs(got[k].cpu().numpy().astype(np.float64) - ref[k]).max(), BAR["obj"])
    if B > 8:
        assert x["ids"][7] == -1 and ref["used"].sum() == B - 1
        assert all(float(got[k][7]) == 0.0 for k in got) and int(used[7]) == 0       # the neighbours were compared above
        assert len(set(x["ids"].tolist())) < B - 1                                   # templates repeat


@pytest.mark.parametrize("V,B,P,seed", CASES)
def test_mesh_metrics_against_fp64(V, B, P, seed):
    gt, pr = make_mesh(B, V, seed)
    ref = mesh_reference(gt, pr, ACC_TH)
    gap_f, gap_p = mesh_gaps(ref)
    print(f"V={V} B={B}: smallest relative gap to an F-score threshold {gap_f:.2e}, to a PCK threshold {gap_p:.2e}")
    assert gap_f > NEAR and gap_p > NEAR                                             # every sample, every threshold
    d0, d1, f0, f1, al = ops.eval_mesh(dev(pr), dev(gt), F_TH, want_aligned=True)
    n = lambda t: t.cpu().numpy().astype(np.float64)
    tag = f"V={V} B={B}"
    held(f"{tag} vertex distances", np.abs(n(d0) - ref["d_raw"]).max(), BAR["mje"])
    held(f"{tag} F-scores", np.abs(n(f0) - ref["fs"]).max(), BAR["fscore"])
    accs = [(d0, ref["measures"])]
    if V >= 3:                                                                       # fewer points fix no similarity (varP = 0 at V = 1)
        held(f"{tag} aligned mesh", np.abs(n(al) - ref["aligned"]).max(), BAR["aligned"])
        held(f"{tag} aligned vertex distances", np.abs(n(d1) - ref["d_al"]).max(), BAR["pamje"])
        held(f"{tag} aligned F-scores", np.abs(n(f1) - ref["fs_al"]).max(), BAR["fscore"])
        accs.append((d1, ref["measures_al"]))
    else:
        assert bool(torch.isfinite(al).all()) and bool(torch.isfinite(d1).all()) and bool(torch.isfinite(f1).all())
    th = ops.eval_thresholds(ACC_TH, DEV)
    for d, (mean, auc, pck) in accs:
        st = ops.eval_accum_init(V, len(ACC_TH), DEV)
        ops.eval_accumulate(st, d, th)
        m = ops.eval_accum_finish(st, V, th).cpu().numpy()
        held(f"{tag} mesh mean", abs(m[0] - mean), BAR["mesh_mean"])
        held(f"{tag} AUC", abs(m[1] - auc), BAR["auc"])
        held(f"{tag} PCK", np.abs(m[2:] - pck).max(), BAR["pck"])
    mje, pamje = ops.eval_hand_joints(dev(pr), dev(gt))[:2]                         # the same kernel's per-sample means
    held(f"{tag} mean distance", np.abs(n(mje) - ref["d_raw"].mean(1)).max(), BAR["mje"])
    if V >= 3:
        held(f"{tag} mean aligned distance", np.abs(n(pamje) - ref["d_al"].mean(1)).max(), BAR["pamje"])


# ---- 3. Procrustes -----------------------------------------------------------------------------------------------------------------
PROCRUSTES_B, PROCRUSTES_SEED = 12, 0


def make_procrustes(n, seed):
    """A (B,n,3) and B = a scaled, rotated, translated copy of A plus 1 mm noise; then every third A mirrored in x"""
    r = np.random.default_rng(seed)
    A = 0.05 * r.standard_normal((PROCRUSTES_B, n, 3))
    R = np_rodrigues(1.0 * r.standard_normal((PROCRUSTES_B, 3)))
    s = r.uniform(0.7, 1.4, PROCRUSTES_B)
    Bp = s[:, None, None] * (A @ np.transpose(R, (0, 2, 1))) + 0.1 * r.standard_normal((PROCRUSTES_B, 1, 3)) \
        + 1e-3 * r.standard_normal((PROCRUSTES_B, n, 3))
    mirrored = np.zeros(PROCRUSTES_B, bool)
    mirrored[2::3] = True
    A[mirrored, :, 0] *= -1.0
    return A.astype(np.float32), Bp.astype(np.float32), mirrored


@pytest.mark.parametrize("n", [21, 778])
def test_procrustes(n):
    A, Bp, mirrored = make_procrustes(n, PROCRUSTES_SEED)
    ref = [np_procrustes(A[b], Bp[b]) for b in range(PROCRUSTES_B)]
    sv = np.stack([r[4] for r in ref])
    print(f"n={n}: sigma3/sigma1 in [{(sv[:, 2] / sv[:, 0]).min():.3e}, {(sv[:, 2] / sv[:, 0]).max():.3e}], mirrored (sigma2-sigma3)/sigma1 >= "
          f"{((sv[:, 1] - sv[:, 2]) / sv[:, 0])[mirrored].min():.3e}")
    assert bool((((sv[:, 1] - sv[:, 2]) / sv[:, 0])[mirrored] > 1e-2).all()) and bool((sv[:, 2] / sv[:, 0] > 1e-3).all())   # every sample
    assert np.array_equal(np.array([r[5] for r in ref]), mirrored)                  # fp64 takes the reflection branch exactly there
    mje, pamje, al, xf = ops.eval_hand_joints(dev(A), dev(Bp), want_aligned=True, want_transform=True)
    xf, al = xf.cpu().numpy(), al.cpu().numpy().astype(np.float64)
    held(f"n={n} aligned", np.abs(al - np.stack([r[3] for r in ref])).max(), BAR["aligned"])
    held(f"n={n} c", np.abs(xf[:, 0] - np.array([r[0] for r in ref])).max(), BAR["xform"])
    held(f"n={n} R", np.abs(xf[:, 1:10].reshape(-1, 3, 3) - np.stack([r[1] for r in ref])).max(), BAR["xform"])
    held(f"n={n} t", np.abs(xf[:, 10:] - np.stack([r[2] for r in ref])).max(), BAR["xform"])
    held(f"n={n} |det R - 1|", np.abs(np.linalg.det(xf[:, 1:10].reshape(-1, 3, 3)) - 1.0).max(), 1e-9)       # a rotation, mirrored or not
    res = np.array([np.linalg.norm(r[3] - Bp[b], axis=1).mean() for b, r in enumerate(ref)])
    held(f"n={n} residual", np.abs(pamje.cpu().numpy() - res).max(), BAR["pamje"])
    assert bool((res[mirrored] > 10 * res[~mirrored].max()).all())                  # no rotation undoes a mirror: the residual shows the branch


# ---- 4. exact counts ---------------------------------------------------------------------------------------------------------------
EXACT_B, EXACT_V, EXACT_SEED = 2, 778, 1


def test_exact_fscore_and_pck_counts():
    gt, pr = make_mesh(EXACT_B, EXACT_V, EXACT_SEED)
    acc_th = np.linspace(0.0, 0.05, 100)
    ref = mesh_reference(gt, pr, acc_th)
    gap_f, gap_p = mesh_gaps(ref)
    print(f"smallest relative gap to an F-score threshold {gap_f:.2e}, to a PCK threshold {gap_p:.2e}")
    assert gap_f > 1e-5 and gap_p > 1e-5                                            # no distance near any threshold used; none left out
    d0, d1, f0, f1, _ = ops.eval_mesh(dev(pr), dev(gt), F_TH)
    for got, want, k in ((f0, ref["fs"], "F"), (f1, ref["fs_al"], "F aligned")):
        want32 = want.astype(np.float32)                                            # equal counts: the same ratio, rounded to fp32 once
        err = np.abs(got.cpu().numpy().astype(np.float64) - want32.astype(np.float64)).max()
        held(k, err, 1.2e-7)                                                        # one fp32 ulp below 1
    th = ops.eval_thresholds(acc_th, DEV)
    for d, dref in ((d0, ref["d_raw"]), (d1, ref["d_al"])):
        st = ops.eval_accum_init(EXACT_V, 100, DEV)
        ops.eval_accumulate(st, d, th)
        counts = st[16 + 8 * EXACT_V:16 + 8 * EXACT_V + 4 * 100 * EXACT_V].cpu().numpy().view(np.uint32).reshape(100, EXACT_V)
        want = (dref[None] <= acc_th[:, None, None]).sum(1)
        assert np.array_equal(counts, want.astype(np.uint32))
        pck = ops.eval_accum_finish(st, EXACT_V, th).cpu().numpy()[2:]
        held("PCK from equal counts", np.abs(pck - want.sum(1) / (EXACT_B * EXACT_V)).max(), 1e-15)


# ---- 5. / 6. pieces, repeats -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh33():
    gt, pr = make_mesh(33, 778, 5)
    return dev(gt), dev(pr)


def test_accumulator_pieces_give_the_bits_of_one_feed(mesh33):
    gt, pr = mesh33
    d0 = ops.eval_mesh(pr, gt, F_TH)[0]
    th = ops.eval_thresholds(np.linspace(0.0, 0.05, 100), DEV)
    states, outs = [], []
    for cuts in ((1,), (16,), ()):
        st = ops.eval_accum_init(778, 100, DEV)
        lo = 0
        for hi in cuts + (33,):
            ops.eval_accumulate(st, d0[lo:hi], th)
            lo = hi
        states.append(bits(st))
        outs.append(bits(ops.eval_accum_finish(st, 778, th)))
    assert states[0] == states[1] == states[2] and outs[0] == outs[1] == outs[2]
    n = int(np.frombuffer(states[0][:8], np.uint64)[0])
    assert n == 33


def test_two_calls_same_bits(mesh33):
    gt, pr = mesh33
    x = make_object(33, 300, 40, 3)
    oargs = (dev(x["obj_rot"]), dev(x["obj_trans"]), dev(x["rot_gt"]), dev(x["trans_gt"]), dev(x["templates"]), torch.from_numpy(x["ids"]))
    th = ops.eval_thresholds(np.linspace(0.0, 0.05, 100), DEV)

    def accumulate():
        st = ops.eval_accum_init(778, 100, DEV)
        ops.eval_accumulate(st, ops.eval_mesh(pr, gt, F_TH)[1], th)
        return st, ops.eval_accum_finish(st, 778, th)

    for name, fn in (("eval_object", lambda: ops.eval_object(*oargs)),
                     ("eval_hand_joints", lambda: ops.eval_hand_joints(pr[:, :21], gt[:, :21], want_aligned=True, want_transform=True, want_dist=True)),
                     ("eval_mesh", lambda: ops.eval_mesh(pr, gt, F_TH, want_aligned=True)),
                     ("accumulator", accumulate)):
        a, b = fn(), fn()
        assert len(a) == len(b) and all(bits(p) == bits(q) for p, q in zip(a, b)), name


# ---- 7. the Evaluator over both backends ------------------------------------------------------------------------------------------
def _record(setting):
    """two batches of (out, targets, meta, obj_cls) from one small model (ResNet-18, 96 + 32 points, B = 2), outputs on the device"""
    from hoisdf_amd import testing as T
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import Tester
    from hoisdf_amd.nets import mano as MANO
    c = Config()
    c.resnet_type = 18
    c.apply_setting(setting)
    c.eval_mesh = setting == "dexycb"                      # the mesh and F-score blocks too (all that the setting dexycb_full adds to dexycb)
    c.num_samp_hand, c.num_samp_obj = 96, 32
    torch.manual_seed(0)
    tester = Tester(c, torch.device("cuda", 0))
    ml = MANO.ManoLayer(MANO.synthetic_assets(0)).to(DEV)
    rec = []
    for it in range(2):
        inputs, targets, meta = T.synthetic_batch(2, 96, 32, seed=5 + it)
        out = tester.predict(inputs, targets, meta, mano_layer=ml)
        rec.append(({k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}, targets, meta, (torch.arange(2) + it) % 4))
    g = torch.Generator().manual_seed(0)
    return c, (0.05 * torch.randn(4, 500, 3, generator=g)).to(DEV), rec


@pytest.fixture(scope="module", params=["dexycb", "ho3d_render"])
def recorded(request, tmp_path_factory):
    c, templates, rec = _record(request.param)
    dirs = {}
    for name, native in (("torch", False), ("native", True), ("native2", True)):
        ev = M.Evaluator(c, templates, native=native)
        for out, targets, meta, obj_cls in rec:
            ev.feed(out, targets, meta, obj_cls)
        dirs[name] = str(tmp_path_factory.mktemp(f"{request.param}_{name}"))
        assert ev.write(dirs[name]) == os.path.join(dirs[name], "results.txt")
    torch.cuda.synchronize()
    return request.param, dirs


_NUM = r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|nan|inf)"


def parse_results(text):
    """results.txt -> (layout: every line with its numbers replaced by '#', the numbers in order)"""
    nums, layout = [], []
    for line in text.splitlines():
        if " :  " in line:                                                           # "key :  value"
            k, v = line.split(" :  ")
            layout.append(k + " :  #")
            nums.append((k, float(v)))
        else:
            found = re.findall(r"(auc|mean_vert3d_avg|F@[\d.]+mm|F_aligned@[\d.]+mm)\s*=\s*(" + _NUM + ")", line)
            layout.append(re.sub(r"=\s*" + _NUM, "=#", line))
            nums += [(k.split("@")[0], float(v)) for k, v in found]
    return layout, nums


# results.txt prints key : value lines in cm at full precision, auc and F-scores with 3 decimals, mean_vert3d_avg in cm with 2: a printed
# number may differ by the bar in its own unit plus, for the rounded ones, one step of the last printed digit
FILE_BAR = {"ADDS_error": 100 * 2e-6, "MME_error": 100 * 2e-6, "OCE_error": 100 * 2e-6, "MCE_error": 100 * 2e-6, "mano_mje": 100 * 1e-7,
            "mano_pamje": 100 * 1e-6, "auc": 1e-6 + 1.001e-3, "mean_vert3d_avg": 100 * 1e-8 + 1.001e-2, "F": 1e-6 + 1.001e-3,
            "F_aligned": 1e-6 + 1.001e-3}


def test_evaluator_backends_write_the_same_file(recorded):
    setting, dirs = recorded
    a, b = (open(os.path.join(dirs[k], "results.txt")).read() for k in ("torch", "native"))
    print(a, b, sep="\n--- native ---\n")
    (la, na), (lb, nb) = parse_results(a), parse_results(b)
    assert la == lb and [k for k, _ in na] == [k for k, _ in nb] and len(na) >= 2   # keys, order and block layout
    if setting == "dexycb":
        assert "Evaluation 3D MESH ALIGNED results:" in la and "F-scores" in la and any(l.startswith("mano_pamje") for l in la)
    else:
        assert la == ["ADDS_error :  #", "MME_error :  #"]
    for (k, x), (_, y) in zip(na, nb):
        held(f"{setting} {k}", abs(x - y), FILE_BAR[k])
    if setting != "dexycb":
        ja, jb = (open(os.path.join(dirs[k], "pred_mano.json")).read() for k in ("torch", "native"))
        assert ja == jb and len(json.loads(ja)[0]) == 4


def test_two_native_evaluators_write_the_same_files(recorded):
    _, dirs = recorded
    for name in sorted(os.listdir(dirs["native"])):
        assert open(os.path.join(dirs["native"], name), "rb").read() == open(os.path.join(dirs["native2"], name), "rb").read(), name


def test_native_evaluator_leaves_unused_samples_out_of_the_object_means(tmp_path):
    """a sample with obj_cls < 0 (HO3D's 019_pitcher_base rule) is no part of ADDS_error / MME_error: the file holds the mean over the
    evaluated samples, as common/metrics.py:131-149 divides by the number of used ones"""
    from hoisdf_amd.config import Config
    B = 12
    x = make_object(B, 50, 8, 9)
    assert x["ids"][7] == -1 and int((x["ids"] >= 0).sum()) == B - 1
    c = Config()
    c.apply_setting("ho3d")
    ev = M.Evaluator(c, dev(x["templates"]), native=True)
    out = {"obj_rot_out": dev(x["obj_rot"]), "obj_trans_out": dev(x["obj_trans"]), "mano_joints_out": torch.zeros(B, 21, 3, device=DEV),
           "mano_mesh_out": torch.zeros(B, 778, 3, device=DEV)}
    ev.feed(out, {"obj_rot": torch.from_numpy(x["rot_gt"]), "rel_obj_trans": torch.from_numpy(x["trans_gt"])}, {"mano_root": torch.zeros(B, 3)},
            torch.from_numpy(x["ids"]))
    _, nums = parse_results(open(ev.write(str(tmp_path))).read())
    ref = np_object(x["obj_rot"], x["obj_trans"], x["rot_gt"], x["trans_gt"], x["templates"], x["ids"])
    used = ref["used"] == 1
    assert [k for k, _ in nums] == ["ADDS_error", "MME_error"]
    held("ADDS_error over the used samples [cm]", abs(nums[0][1] - 100 * ref["adds"][used].mean()), 100 * BAR["obj"])
    held("MME_error over the used samples [cm]", abs(nums[1][1] - 100 * ref["mme"][used].mean()), 100 * BAR["obj"])


# ---- 8. a plain C host -------------------------------------------------------------------------------------------------------------
def test_c_host_eval(tmp_path):
    """tests/c/test_eval_host.c on a dump of two batches: the bits of the Python calls, and a results.txt with the Evaluator's layout"""
    from hoisdf_amd.config import Config
    B, V, P, T, J, NV, steps = 3, 300, 40, 4, 21, 778, 100
    batches = []
    for it in range(2):
        x = make_object(B, V, P, 20 + it, T=T)
        gt_v, pr_v = make_mesh(B, NV, 30 + it)
        gt_j, pr_j = make_mesh(B, J, 40 + it)
        batches.append((x, gt_j, pr_j, gt_v, pr_v))
    templates = batches[0][0]["templates"]
    src, dst, txt = str(tmp_path / "eval_in.bin"), str(tmp_path / "eval_out.bin"), str(tmp_path / "results.txt")
    with open(src, "wb") as f:
        f.write(struct.pack("<8i", 2, B, P, T, V, J, NV, steps))
        f.write(np.asarray(F_TH, "<f8").tobytes())
        f.write(np.linspace(0.0, 0.05, steps).astype("<f8").tobytes())
        f.write(templates.astype("<f4").tobytes())
        for x, gt_j, pr_j, gt_v, pr_v in batches:
            f.write(x["ids"].astype("<i4").tobytes())
            for a in (x["obj_rot"], x["obj_trans"], x["rot_gt"], x["trans_gt"], pr_j, gt_j, pr_v, gt_v):
                f.write(np.ascontiguousarray(a, "<f4").tobytes())
    # the Python side: the same calls, and an Evaluator fed the same numbers
    c = Config()
    c.apply_setting("dexycb_full")
    ev = M.Evaluator(c, dev(templates), native=True)
    want = []
    for x, gt_j, pr_j, gt_v, pr_v in batches:
        o = ops.eval_object(dev(x["obj_rot"]), dev(x["obj_trans"]), dev(x["rot_gt"]), dev(x["trans_gt"]), dev(templates), torch.from_numpy(x["ids"]))
        h = ops.eval_hand_joints(dev(pr_j), dev(gt_j))[:2]
        m = ops.eval_mesh(dev(pr_v), dev(gt_v), F_TH)[:4]
        want += [bits(t) for t in (*o[:4], *h, *m)] + [bits(o[4])]
        out = {"obj_rot_out": dev(x["obj_rot"]), "obj_trans_out": dev(x["obj_trans"]), "mano_joints_out": dev(pr_j), "mano_joints_gt_out": dev(gt_j),
               "mano_mesh_out": dev(pr_v), "mano_mesh_gt_out": dev(gt_v)}
        ev.feed(out, {"obj_rot": torch.from_numpy(x["rot_gt"]), "rel_obj_trans": torch.from_numpy(x["trans_gt"])},
                {"mano_root": torch.zeros(B, 3)}, torch.from_numpy(x["ids"]).long())
    py_txt = open(ev.write(str(tmp_path / "py"))).read()
    want += [bits(e.measures_device()) for e in (ev.mesh_err, ev.mesh_err_al)]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_eval_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_eval_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe, src, dst, txt], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "c host eval ok" in run.stdout, run.stdout + run.stderr
    assert open(dst, "rb").read() == b"".join(want)
    c_txt = open(txt).read()
    print(py_txt, c_txt, sep="\n--- C host ---\n")
    (lp, nump), (lc, numc) = parse_results(py_txt), parse_results(c_txt)
    assert lp == lc and [k for k, _ in nump] == [k for k, _ in numc]
    for (k, x), (_, y) in zip(nump, numc):
        # key : value lines: the same per-sample fp32 values summed in fp64 in two orders (a torch reduction, a C loop) - 1e-12 relative
        # covers either order's rounding a thousand times over; auc / mean_vert3d_avg are printed from bit-equal doubles; the F lines
        # print a mean of bit-equal fp32 values taken in fp32 by numpy and by the C loop - at most one step of the last printed digit
        tol = 1e-12 * abs(x) if k.endswith("_error") or k.startswith("mano_") else 1.001e-3 if k.startswith("F") else 0.0
        assert abs(x - y) <= tol, (k, x, y)
