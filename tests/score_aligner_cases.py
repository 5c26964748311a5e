"""Inputs and the numpy yardstick of the score_aligner tests (tests/test_score_aligner_abi.py on the CPU, tests/test_gpu_score_aligner*.py on the device).

Inputs: synth.make_workload(4, 20000, seed=3); slice s's fixed cloud is scan i moved by S_s^-1 (points and normals), its moving cloud a stride of the map;
X = x0[i].  The slices: projective 1081 columns with Cauchy 0.05 and sensor offset S0; exact NN with max_distance 0.3 and S1; projective 721 columns with
Cauchy 0.01 and no offset; a fourth slice with the distance-map finder.  Every finder kind but the first sits at a slice index >= 1, so the digest's
salt is exercised.

The yardstick is `combine`: a scored item restated in numpy float32 from per-slice rows -- counts and digests of every slice, the sums of the contributing
slices added in slice order from +0, the prior last (`prior_terms`: the aligner's prior_apply with every product and sum rounded separately; its pose
composition and its sine / cosine are the oracle's own fixed sequences).  Not a test module."""
import ctypes as C
import types

import numpy as np

from srrg2_laser_slam_2d_amd import synth

S_OFF = [(0.1, -0.05, 0.3), (-0.2, 0.0, 3.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
STRIDE = [7, 11, 3, 5]
# (finder kind, canvas columns, max_distance, Cauchy threshold or None)
SLICES = [("proj", 1081, 0.0, 0.05), ("nn", 0, 0.3, None), ("proj", 721, 0.0, 0.01), ("distmap", 0, 0.3, None)]
MIN_CORR = 10
F32 = np.float32


def _move(cloud, pose):
    """(x, y, nx, ny) rows moved by the isometry `pose`, in float32"""
    c, s = F32(np.cos(pose[2])), F32(np.sin(pose[2]))
    out = np.empty_like(cloud)
    out[:, 0] = c * cloud[:, 0] - s * cloud[:, 1] + F32(pose[0]); out[:, 1] = s * cloud[:, 0] + c * cloud[:, 1] + F32(pose[1])
    out[:, 2] = c * cloud[:, 2] - s * cloud[:, 3]; out[:, 3] = s * cloud[:, 2] + c * cloud[:, 3]
    return np.ascontiguousarray(out, F32)


def make_inputs():
    wl = synth.make_workload(4, 20000, seed=3)
    c = types.SimpleNamespace()
    c.n = len(wl.x0)
    c.poses = np.ascontiguousarray(wl.x0, F32)
    scans = [np.ascontiguousarray(wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]], F32) for i in range(c.n)]
    c.fixed = []      # [slice][item]
    for S in S_OFF:
        if S == (0.0, 0.0, 0.0):
            c.fixed.append(scans)
        else:
            inv = synth.invert_poses(np.array([S], np.float64))[0]
            c.fixed.append([_move(sc, inv) for sc in scans])
    c.moving = [np.ascontiguousarray(wl.map_points[::st], F32) for st in STRIDE]
    return c


def oracle_slices(po, min_corr=None):
    """the four slices as oracle SliceParams; min_corr: one value for all, or a list"""
    out = []
    for s, (kind, cols, md, tau) in enumerate(SLICES):
        mc = MIN_CORR if min_corr is None else (min_corr[s] if isinstance(min_corr, (list, tuple)) else min_corr)
        kw = dict(min_num_correspondences=int(mc), sensor_in_robot=S_OFF[s], robustifier=po.ROBUST_NONE if tau is None else po.ROBUST_CAUCHY,
                  chi_threshold=0.05 if tau is None else tau)
        if kind == "proj":
            out.append(po.slice_params(finder=po.FINDER_PROJECTIVE, canvas_cols=cols, **kw))
        elif kind == "nn":
            out.append(po.slice_params(finder=po.FINDER_NN, max_distance=md, **kw))
        else:
            out.append(po.slice_params(finder=po.FINDER_DISTMAP, max_distance=md, resolution=0.05, **kw))
    return out


def _f3(v):
    return np.ascontiguousarray(v, F32).reshape(3)


def inverse(po, a):
    """the oracle's lsmo_inverse_f (= the library's inverse_host)"""
    a = _f3(a); out = np.empty(3, F32)
    fn = po.lib().lsmo_inverse_f; fn.argtypes = [C.c_void_p, C.c_void_p]; fn.restype = None
    fn(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def compose(po, a, b):
    """the oracle's lsmo_compose_f (= the library's compose_host)"""
    a, b = _f3(a), _f3(b); out = np.empty(3, F32)
    fn = po.lib().lsmo_compose_f; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; fn.restype = None
    fn(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def effective_pose(po, S, X):
    """Xe = X bit for bit when S compares equal to (0, 0, 0), else S^-1 X"""
    X = _f3(X)
    if all(F32(v) == F32(0.0) for v in S):
        return X.copy()
    return compose(po, inverse(po, S), X)


def prior_terms(po, z, omega, X):
    """(Hp [9], bp [3]) the aligner's prior adds: e = t2v(Z^-1 X), J = blkdiag(R_e, 1); J^T Omega J and J^T Omega e, every product and sum rounded
    separately in the device function's order (sums start at +0); omega as given, symmetric or not"""
    E = compose(po, inverse(po, z), X)
    s_, c = po.sincos(E[2]); s_, c = F32(s_[0]), F32(c[0])
    om = np.ascontiguousarray(omega, F32).reshape(9)
    Jp = np.array([c, -s_, 0.0, s_, c, 0.0, 0.0, 0.0, 1.0], F32)
    OJ = np.zeros(9, F32); Oe = np.zeros(3, F32)
    for r in range(3):
        v = F32(0.0)
        for k in range(3):
            v = F32(v + F32(om[3 * r + k] * E[k]))
        Oe[r] = v
        for cc in range(3):
            v = F32(0.0)
            for k in range(3):
                v = F32(v + F32(om[3 * r + k] * Jp[3 * k + cc]))
            OJ[3 * r + cc] = v
    Hp = np.zeros(9, F32); bp = np.zeros(3, F32)
    for r in range(3):
        for cc in range(3):
            v = F32(0.0)
            for k in range(3):
                v = F32(v + F32(Jp[3 * k + r] * OJ[3 * k + cc]))
            Hp[3 * r + cc] = v
        v = F32(0.0)
        for k in range(3):
            v = F32(v + F32(Jp[3 * k + r] * Oe[k]))
        bp[r] = v
    return Hp, bp


def combine(po, rows, min_corr, X, prior=None):
    """rows: per slice (H [3, 3], b [3], n_corr, n_in, n_out, chi_in, chi_out, digest with the slice's salt); min_corr: per slice.
    Returns dict(H [3, 3], b [3], n_corr, n_in, n_out, chi_in, chi_out, digest, active)."""
    H = np.zeros(9, F32); b = np.zeros(3, F32); chi_in = F32(0.0); chi_out = F32(0.0)
    n_corr = n_in = n_out = active = 0; dig = 0
    for (Hs, bs, nc, ni, no, ci, co, dg), mc in zip(rows, min_corr):
        n_corr += int(nc); dig = (dig + int(dg)) & 0xFFFFFFFFFFFFFFFF
        if int(nc) <= int(mc):
            continue
        H = (H + np.ascontiguousarray(Hs, F32).reshape(9)).astype(F32); b = (b + np.ascontiguousarray(bs, F32).reshape(3)).astype(F32)
        chi_in = F32(chi_in + F32(ci)); chi_out = F32(chi_out + F32(co)); n_in += int(ni); n_out += int(no); active += 1
    if prior is not None and active:
        Hp, bp = prior_terms(po, prior[0], prior[1], X)
        H = (H + Hp).astype(F32); b = (b + bp).astype(F32)
    return dict(H=H.reshape(3, 3), b=b, n_corr=n_corr, n_in=n_in, n_out=n_out, chi_in=chi_in, chi_out=chi_out, digest=dig, active=active)


def oracle_row(po, sp, s, fixed, moving, Xe, order):
    """slice s's row from the CPU oracle at Xe: po.find, then the sequential po.linearize ("sum_order" 1) or po.linearize_device_order (0)"""
    pairs = po.find(sp, fixed, moving, Xe)
    H, b, st = (po.linearize if order else po.linearize_device_order)(sp, fixed, moving, pairs, Xe)
    return (H, b, len(pairs), st.n_in, st.n_out, st.chi_in, st.chi_out, po.pair_digest(pairs, s))


def asym_prior(X, seed=0):
    """the tests' prior: Omega = L L^T made asymmetric in one entry, mean turned 0.01 rad from X"""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.uniform(0.5, 2.0, (3, 3))) * np.array([[30.0, 1.0, 1.0], [1.0, 30.0, 1.0], [1.0, 1.0, 20.0]])
    om = (L @ L.T).astype(F32)
    om[0, 2] = F32(om[0, 2] * 1.25 + 3.0)
    z = _f3(X).copy(); z[2] = F32(z[2] + F32(0.01))
    return z, om


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)
