"""Float64 restatement of the point-cloud augmentation (csrc/pcl_augment.h) -- TEST INFRASTRUCTURE, independent of
``PclAugment.apply``: plain loops over envs and objects, numpy over the points, every draw from
``oracle.token_dropout.tok_hash`` and the ``gauss`` / ``threshold`` of tests/img_augment_ref.py.

Sites and planes are those tabled in the header.  ``g = env * P_total + p`` numbers a point (p over the env's objects),
``g * 3 + c`` a coordinate; outlier k of object o uses the numbers of point ``off[o] + k``.  Per-episode draws hash
``se = seed_episode + (episode[env] << 32)`` (mod 2^64); everything else hashes ``seed_step``."""
import math

import numpy as np
import torch

from oracle.token_dropout import tok_hash
from tests.img_augment_ref import gauss, threshold

PLANE_PN, PLANE_JITTER, PLANE_FREE, PLANE_CONTOUR = 3, 4, 5, 6
SITE_HIT, SITE_ANGLE, SITE_AXIS, SITE_MASK, SITE_CONTOUR, SITE_SIDE, SITE_INDEX, SITE_EXEMPT, SITE_DROP = range(14, 23)

DEFAULTS = dict(sigma=0.001, noise_clip=0.001, const_noise=0.001, noise_prob=0.3, hit_prob=0.7, rot_deg=0.0,
                outlier_ratio=0.0, contour_prob=0.75, outlier_scale=1.5, dropout_ratio=0.0, no_dropout_prob=0.8)
ORDER = ("sigma", "noise_clip", "const_noise", "noise_prob", "hit_prob", "rot_deg", "outlier_ratio", "contour_prob",
         "outlier_scale", "dropout_ratio", "no_dropout_prob")


def params(**kw):
    """The op's ``params`` list, the defaults of ``PclAugment`` with ``kw`` over them."""
    q = {**DEFAULTS, **kw}
    return [float(q[k]) for k in ORDER]


def f32(v):
    return float(np.float32(v))


def event(h, p):
    """hash < threshold(p), the 64-bit threshold: p = 1 is "always"."""
    return np.asarray(h).astype(np.int64) < threshold(p)


def episode_seed(seed_episode, ep):
    return (int(seed_episode) + ((int(ep) & 0xFFFFFFFF) << 32)) & 0xFFFFFFFFFFFFFFFF


def episode_params(seed_episode, env, ep, rot_deg):
    """(angle in degrees, axis, pn (3,)) of env ``env`` in its episode ``ep``."""
    se = episode_seed(seed_episode, ep)
    u = float(tok_hash(se, SITE_ANGLE, [env])[0] >> np.uint32(8)) * 2.0 ** -24
    axis = (int(tok_hash(se, SITE_AXIS, [env])[0] >> np.uint32(8)) * 3) >> 24
    pn = gauss(se, PLANE_PN, (3 * (env + 1),)).numpy()[3 * env:]
    return (2.0 * u - 1.0) * f32(rot_deg), axis, pn


def const_offset(pn, const_noise, noise_clip):
    """The per-env offset of stage a: clamp(const_noise pn, +-noise_clip)."""
    return np.clip(f32(const_noise) * np.asarray(pn, dtype=np.float64), -f32(noise_clip), f32(noise_clip))


def rotate(x, angle_rad, axis):
    """(P, 3) row vectors times the axis matrix of PointCloudAugmentations.random_rotate."""
    c, s = math.cos(angle_rad), math.sin(angle_rad)
    rot = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]],
           2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return x @ np.array(rot, dtype=np.float64)


def augment(clouds, points, episode, q, seed_episode, seed_step):
    """``clouds`` (N, ...) of N * sum(points) * 3 values, ``q`` the op's ``params`` list -> (float64 tensor of clouds'
    shape, events).  events: hit (N,), mask / drop / replaced (N, P_total) bool, winner (N, P_total) int (-1 = none),
    axis (N,), angle_deg (N,), exempt (N, objects), contour / index (N, P_total) per outlier slot (-1 / False past K),
    after_noise / after_rot (N, P_total, 3): the cloud between the stages (the input where the env is missed)."""
    q = dict(zip(ORDER, q))
    N, Pt = clouds.shape[0], sum(points)
    x = clouds.detach().cpu().double().numpy().reshape(N, Pt, 3)
    ep = episode.detach().cpu().numpy()
    sigma, clip, cn = f32(q["sigma"]), f32(q["noise_clip"]), f32(q["const_noise"])
    n_el = N * Pt
    h_mask, h_drop = tok_hash(seed_step, SITE_MASK, np.arange(n_el)), tok_hash(seed_step, SITE_DROP, np.arange(n_el))
    h_contour, h_index = tok_hash(seed_step, SITE_CONTOUR, np.arange(n_el)), tok_hash(seed_step, SITE_INDEX, np.arange(n_el))
    h_side = tok_hash(seed_step, SITE_SIDE, np.arange(n_el * 3)).reshape(n_el, 3)
    z_jit = gauss(seed_step, PLANE_JITTER, (n_el, 3)).numpy()
    z_free = gauss(seed_step, PLANE_FREE, (n_el, 3)).numpy()
    z_cont = gauss(seed_step, PLANE_CONTOUR, (n_el, 3)).numpy()
    ev = dict(hit=event(tok_hash(seed_step, SITE_HIT, np.arange(N)), q["hit_prob"]),
              mask=np.zeros((N, Pt), bool), drop=np.zeros((N, Pt), bool), replaced=np.zeros((N, Pt), bool),
              winner=np.full((N, Pt), -1), axis=np.zeros(N, int), angle_deg=np.zeros(N), exempt=np.zeros((N, len(points)), bool),
              contour=np.zeros((N, Pt), bool), index=np.full((N, Pt), -1), pn=np.zeros((N, 3)),
              after_noise=x.copy(), after_rot=x.copy())
    out = x.copy()
    for env in range(N):
        if not ev["hit"][env]:
            continue
        deg, axis, pn = episode_params(seed_episode, env, ep[env], q["rot_deg"])
        ev["axis"][env], ev["angle_deg"][env], ev["pn"][env] = axis, deg, pn
        off = 0
        for o, P in enumerate(points):
            g = env * Pt + off + np.arange(P)
            y = x[env, off:off + P].copy()
            # a. noise
            mask = event(h_mask[g], q["noise_prob"]) if sigma > 0 else np.zeros(P, bool)
            ev["mask"][env, off:off + P] = mask
            y = y + np.clip(sigma * z_jit[g], -clip, clip) * mask[:, None]
            y = y + const_offset(pn, q["const_noise"], q["noise_clip"])[None]
            ev["after_noise"][env, off:off + P] = y
            # b. rotation
            if q["rot_deg"] > 0:
                y = rotate(y, deg * (math.pi / 180), axis)
            ev["after_rot"][env, off:off + P] = y
            # c. outliers
            K = int(P * q["outlier_ratio"])
            if K > 0:
                lo, hi = y.min(0), y.max(0)
                gk = g[:K]
                contour = event(h_contour[gk], q["contour_prob"])
                index = ((h_index[gk] >> np.uint32(8)).astype(np.int64) * P) >> 24
                ev["contour"][env, off:off + K], ev["index"][env, off:off + K] = contour, index
                side = event(h_side[gk], 0.5)
                beyond = np.abs(z_cont[gk])
                new = np.where(contour[:, None], np.where(side, hi + beyond, lo - beyond), f32(q["outlier_scale"]) * z_free[gk])
                for k in range(K):                                # in rising k: the highest k wins
                    y[index[k]] = new[k]
                    ev["winner"][env, off + index[k]] = k
                ev["replaced"][env, off:off + P] = ev["winner"][env, off:off + P] >= 0
            # d. dropout
            if q["dropout_ratio"] > 0:
                h_ex = tok_hash(seed_step, SITE_EXEMPT, [env * 4 + o])[0]
                exempt = not bool(event(h_ex, f32(1.0 - q["no_dropout_prob"])))
                ev["exempt"][env, o] = exempt
                drop = event(h_drop[g], q["dropout_ratio"]) & (not exempt)
                ev["drop"][env, off:off + P] = drop
                y[drop] = 0.0
            out[env, off:off + P] = y
            off += P
    return torch.from_numpy(out).reshape(clouds.shape), ev


# ---- the bounds of the issue, per coordinate -------------------------------------------------------------------------
def bound_noise(x, q):
    """N = 2e-5 (sigma + const_noise) + 2^-22 (|x| + 2 noise_clip)."""
    q = dict(zip(ORDER, q))
    return 2e-5 * (q["sigma"] + q["const_noise"]) + 2.0 ** -22 * (np.abs(x) + 2 * q["noise_clip"])


def bound_rot(x, axis, q, x_in=None):
    """R = 2^-20 (|a| + |b|) + 1.5 N over (N, P, 3) inputs ``x`` (the cloud BEFORE the rotation, i.e. after the noise):
    a, b the two input coordinates that enter a sum; N (of the stage-a input ``x_in``) taken at the larger of them.  The
    coordinate on the axis: N."""
    n = bound_noise(x if x_in is None else x_in, q)
    out = np.empty_like(x)
    for env in range(x.shape[0]):
        a = int(axis[env])
        i, j = [c for c in range(3) if c != a]
        s = np.abs(x[env, :, i]) + np.abs(x[env, :, j])
        r = 2.0 ** -20 * s + 1.5 * np.maximum(n[env, :, i], n[env, :, j])
        out[env, :, a] = n[env, :, a]
        out[env, :, i] = r
        out[env, :, j] = r
    return out


def tolerance(clouds, points, q, ev, out):
    """The issue's bound of every coordinate of an fp32 result against ``out`` = the restatement's: 0 where the value is
    copied or zeroed (missed envs, dropped points), N after the noise alone, R after the rotation, and on replaced points
    O = max R over the cloud + 2e-5 max(1, outlier_scale) + 2^-22 |value|."""
    qd = dict(zip(ORDER, q))
    N, Pt = clouds.shape[0], sum(points)
    x = clouds.detach().cpu().double().numpy().reshape(N, Pt, 3)
    out = out.detach().cpu().double().numpy().reshape(N, Pt, 3)
    tol = bound_noise(x, q)
    if qd["rot_deg"] > 0:
        tol = bound_rot(ev["after_noise"], ev["axis"], q, x)
    off = 0
    for P in points:
        sl = slice(off, off + P)
        cloud_max = tol[:, sl].max(axis=(1, 2), keepdims=True)
        o = cloud_max + 2e-5 * max(1.0, qd["outlier_scale"]) + 2.0 ** -22 * np.abs(out[:, sl])
        tol[:, sl] = np.where(ev["replaced"][:, sl, None], o, tol[:, sl])
        off += P
    tol[ev["drop"]] = 0.0
    tol[~ev["hit"]] = 0.0
    return torch.from_numpy(tol).reshape(clouds.shape)


def check(got, clouds, points, q, ev, out):
    """max over coordinates of |got - out| / tolerance (0 / 0 counts as 0, x / 0 as inf): <= 1 passes."""
    tol = tolerance(clouds, points, q, ev, out)
    err = (got.detach().cpu().double() - out).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(ratio.max())
