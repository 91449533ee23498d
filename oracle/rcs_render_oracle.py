"""CPU restatement of the depth ray-caster (TEST INFRASTRUCTURE; see oracle/rcs_oracle.h for the rules).

numpy, one ray per pixel, the same shapes and the same formulas as csrc/render.h; the frames come from the oracle's
mjData restatement (xpos / xmat of the last position stage).  What is restated from the reference -- the camera model
of MuJoCo, the OpenGL depth encoding, python/rcs/camera/sim.py:57-115 (row flip, metres in float32, uint16
millimetres, intrinsics, extrinsics) -- is cited in csrc/render.h and rcs_amd/camera.py.  PARITY UNPINNED for the
pixels themselves: the reference's come from MuJoCo's OpenGL rasteriser over the visual meshes.
"""

from __future__ import annotations

import numpy as np

SHAPE_PLANE, SHAPE_BOX, SHAPE_HULL, SHAPE_CAPSULE = 0, 1, 2, 3
last_hit_shape = None
last_hit_normal = None


def oracle_frames(osim, cm) -> dict:
    """link index -> (R [3,3], p [3]) from the oracle's mjData: robot links, -1 world, -2 the free box."""
    d = osim.s.d
    xpos = np.ctypeslib.as_array(d.xpos)
    xmat = np.ctypeslib.as_array(d.xmat)
    frames = {-1: (np.eye(3), np.zeros(3))}
    for j in range(cm.njnt):
        b = int(cm.arrays["jnt_bodyid"][j])
        frames[j] = (xmat[b].reshape(3, 3).copy(), xpos[b].copy())
    if getattr(cm, "free_bodies", []):
        w, x, y, z = d.box.xquat[:]
        R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
        frames[-2] = (R, np.array(d.box.xpos[:]))
    return frames


def _cast(x, T):
    """An input in the arithmetic type T (through float64: what the tables hold)."""
    return np.asarray(x, dtype=np.float64).astype(T)


def _is(T, *arrays):
    """No intermediate was silently promoted: every one of `arrays` has the arithmetic type."""
    for a in arrays:
        assert a.dtype == T, (a.dtype, T)


def render_depth(rs, cam, frames, colour=False, offset=(0.0, 0.0), dtype=np.float64, detail=False):
    """rs: rcs_amd.render.RenderScene; cam: (link, pos, rot9, fovy_deg, W, H).  Returns (depth_gl [H,W] float32 rows
    bottom-up, depth_mm [H,W] uint16 rows top-down, cam_R, cam_p) and, with `colour`, rgb [H,W,3] uint8 rows bottom-up:
    the colour of the shape entered first, flat-shaded on the entry face (csrc/render.h, COLOR).

    `offset` = (dx, dy) in pixels is added to every pixel centre before the rays are built: the restatement beside the
    centres (tests/render_cases.py asks it whether a pixel's answer is decided).  `dtype` is the arithmetic type: every input
    is cast to it and the same formulas run in it (float32: what float32 rays cost, measured, not assumed).  With `detail`
    the result is a dict: the above (colour included) plus, rows bottom-up, hit [H,W] bool, shape [H,W] (index of the shape
    entered first, -1: none), normal [H,W,3] (the entry face's, shape frame), face [H,W] (which face: 0 the plane; box
    2 * axis + side; hull: its plane's index; capsule: 0 wall, 1 / 2 the cap at -z / +z), z [H,W] (view depth of the hit,
    zfar without one), checker [H,W] bool (the second colour of a checkered shape) and ray [H,W,3] (direction, world)."""
    T = np.dtype(dtype).type
    link, cpos, crot, fovy, W, H = cam
    fr = {k: (_cast(R, T), _cast(p, T)) for k, (R, p) in frames.items()}
    Rl, pl = fr[link]
    cR, cp = Rl @ _cast(crot, T).reshape(3, 3), Rl @ _cast(cpos, T) + pl
    ty = np.tan(T(fovy) * T(np.pi) / T(360.0))
    tx = ty * T(W) / T(H)
    col, row = np.meshgrid(np.arange(W).astype(T), np.arange(H).astype(T))
    dc = np.stack([(T(2) * (col + T(0.5) + T(offset[0])) / T(W) - T(1)) * tx, (T(2) * (row + T(0.5) + T(offset[1])) / T(H) - T(1)) * ty,
                   -np.ones((H, W), dtype=T)], axis=-1)
    d = dc @ cR.T
    dd = (d * d).sum(-1)
    _is(T, cR, cp, ty, tx, dc, d, dd)
    znear, zfar = T(rs.znear), T(rs.zfar)
    r_pos, r_rot, r_size, r_sphere, r_planes = _cast(rs.pos, T), _cast(rs.rot, T), _cast(rs.size, T), _cast(rs.sphere, T), _cast(rs.planes, T)
    best = np.full((H, W), zfar)
    hit = np.zeros((H, W), dtype=bool)
    hit_g = np.full((H, W), -1)
    hit_f = np.zeros((H, W), dtype=np.int64)
    hit_n = np.zeros((H, W, 3), dtype=T)  # entry face normal, shape frame
    up = np.array([0.0, 0.0, 1.0], dtype=T)
    for g in range(len(rs.shape)):
        Rg, pg = fr[int(rs.link[g])]
        R, p = Rg @ r_rot[g].reshape(3, 3), Rg @ r_pos[g] + pg
        live = np.ones((H, W), dtype=bool)
        if r_sphere[g][3] >= 0:
            oc = R @ r_sphere[g][:3] + p - cp
            b = d @ oc
            live = ~((oc @ oc) * dd - b * b > r_sphere[g][3] ** 2 * dd)
        lo = R.T @ (cp - p)
        ld = d @ R
        t0 = np.full((H, W), znear)
        t1 = best.copy()
        _is(T, R, p, lo, ld, t0, t1)
        if rs.shape[g] == SHAPE_PLANE:
            ok = live & (ld[..., 2] < 0) & (lo[2] > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -lo[2] / ld[..., 2]
            ok &= (t >= t0) & (t < t1)
            best = np.where(ok, t, best)
            hit |= ok
            hit_g = np.where(ok, g, hit_g)
            hit_f = np.where(ok, 0, hit_f)
            hit_n = np.where(ok[..., None], up, hit_n)
            _is(T, best, hit_n)
            continue
        ok = live.copy()
        face_n = np.zeros((H, W, 3), dtype=T)
        face_i = np.zeros((H, W), dtype=np.int64)
        if rs.shape[g] == SHAPE_CAPSULE:
            # axis z of the shape frame, radius size[0], half length size[2] - size[0]: the first point of the ray on the wall
            # between the caps or on the outer half of a cap sphere
            r, hl = r_size[g][0], r_size[g][2] - r_size[g][0]
            with np.errstate(divide="ignore", invalid="ignore"):
                a = ld[..., 0] ** 2 + ld[..., 1] ** 2
                bq = lo[0] * ld[..., 0] + lo[1] * ld[..., 1]
                cq = lo[0] ** 2 + lo[1] ** 2 - r * r
                disc = bq * bq - a * cq
                t = (-bq - np.sqrt(disc)) / a
                te = np.where((a > 0) & (disc >= 0) & (np.abs(lo[2] + t * ld[..., 2]) <= hl), t, T(np.inf))
                A = a + ld[..., 2] ** 2
                for zc in (-hl, hl):
                    oz = lo[2] - zc
                    B, Cq = bq + oz * ld[..., 2], cq + oz * oz
                    ds = B * B - A * Cq
                    t = (-B - np.sqrt(ds)) / A
                    zr = oz + t * ld[..., 2]
                    te = np.where((ds >= 0) & ((zr >= 0) if zc > 0 else (zr <= 0)) & (t < te), t, te)
            ok &= np.isfinite(te) & (te > znear) & (te < best)
            hp = lo + np.where(ok, te, T(0))[..., None] * ld
            face_n = hp.copy()
            face_n[..., 2] = hp[..., 2] - np.clip(hp[..., 2], -hl, hl)
            best = np.where(ok, te, best)
            hit |= ok
            hit_g = np.where(ok, g, hit_g)
            hit_f = np.where(ok, np.where(face_n[..., 2] < 0, 1, np.where(face_n[..., 2] > 0, 2, 0)), hit_f)
            hit_n = np.where(ok[..., None], face_n, hit_n)
            _is(T, te, best, hit_n)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            if rs.shape[g] == SHAPE_BOX:
                for k in range(3):
                    zero = ld[..., k] == 0
                    inv = T(1) / ld[..., k]
                    ta, tb = (-r_size[g][k] - lo[k]) * inv, (r_size[g][k] - lo[k]) * inv
                    ta, tb = np.minimum(ta, tb), np.maximum(ta, tb)
                    t0n, t1n = np.maximum(t0, ta), np.minimum(t1, tb)
                    axis = np.zeros(3, dtype=T)
                    axis[k] = 1.0
                    enters = ~(zero | ~ok) & (ta > t0)
                    face_n = np.where(enters[..., None], np.where(ld[..., k] > 0, T(-1), T(1))[..., None] * axis, face_n)
                    face_i = np.where(enters, np.where(ld[..., k] > 0, 2 * k, 2 * k + 1), face_i)
                    t0, t1 = np.where(zero | ~ok, t0, t0n), np.where(zero | ~ok, t1, t1n)
                    ok &= np.where(zero, abs(lo[k]) <= r_size[g][k], t0 <= t1)
            else:
                for k, pl4 in enumerate(r_planes[rs.plane_adr[g]: rs.plane_adr[g] + rs.plane_num[g]]):
                    nd = ld @ pl4[:3]
                    no = pl4[3] - pl4[:3] @ lo
                    zero = nd == 0
                    t = no / nd
                    t0n = np.where(nd < 0, np.maximum(t0, t), t0)
                    t1n = np.where(nd > 0, np.minimum(t1, t), t1)
                    enters = ~(zero | ~ok) & (nd < 0) & (t > t0)
                    face_n = np.where(enters[..., None], pl4[:3], face_n)
                    face_i = np.where(enters, k, face_i)
                    t0, t1 = np.where(zero | ~ok, t0, t0n), np.where(zero | ~ok, t1, t1n)
                    ok &= np.where(zero, no >= 0, t0 <= t1)
        ok &= (t0 > znear) & (t0 < best)
        best = np.where(ok, t0, best)
        hit |= ok
        hit_g = np.where(ok, g, hit_g)
        hit_f = np.where(ok, face_i, hit_f)
        hit_n = np.where(ok[..., None], face_n, hit_n)
        _is(T, t0, t1, best, hit_n)
    global last_hit_shape, last_hit_normal
    last_hit_shape = hit_g  # [H, W] index of the shape each ray enters first (-1: none), rows bottom-up: for the tests' bookkeeping
    last_hit_normal = hit_n  # [H, W, 3] the entry face's normal in that shape's frame
    inv_near, inv_far = T(1) / znear, T(1) / zfar
    enc = np.where(hit, (inv_near - T(1) / best) / (inv_near - inv_far), T(1))
    _is(T, enc)
    dgl = enc.astype(np.float32)
    # python/rcs/camera/sim.py:57-86 on the buffer mjr_readPixels returned
    frame = dgl[::-1]
    with np.errstate(invalid="ignore"):  # (a millimetre value beyond uint16: the cast is not defined, nobody may read it)
        z = np.float32(rs.znear) / (np.float32(1) - frame * np.float32(1 - rs.znear / rs.zfar))
        mm = (z * np.float32(1000)).astype(np.uint16)
    if not colour and not detail:
        return dgl, mm, cR, cp
    rgb, checker = shade(rs, frames, dict(ray=d, hit=hit, shape=hit_g, normal=hit_n, z=best, cam_p=cp), dtype=dtype)
    if not detail:
        return dgl, mm, cR, cp, rgb
    return dict(depth_gl=dgl, depth_mm=mm, cam_R=cR, cam_p=cp, rgb=rgb, hit=hit, shape=hit_g, normal=hit_n, face=hit_f, z=best, checker=checker, ray=d)


def shade(rs, frames, det, dtype=np.float64):
    """The colour stage on what the rays found (`det`: ray, hit, shape, normal, z, cam_p of render_depth's detail):
    (rgb [H,W,3] uint8 rows bottom-up, checker [H,W] bool)."""
    T = np.dtype(dtype).type
    d, hit, hit_g, hit_n, best, cp = det["ray"], det["hit"], det["shape"], det["normal"], det["z"], det["cam_p"]
    H, W = hit.shape
    fr = {k: (_cast(R, T), _cast(p, T)) for k, (R, p) in frames.items()}
    r_pos, r_rot, r_col = _cast(rs.pos, T), _cast(rs.rot, T), _cast(rs.colour, T)
    dd = (d * d).sum(-1)
    inv_len = T(1) / np.sqrt(dd)
    f = T(0.5) * (d[..., 2] * inv_len + T(1))
    sky1, sky2 = _cast(rs.sky_rgb1, T), _cast(rs.sky_rgb2, T)
    out = sky2 + f[..., None] * (sky1 - sky2)
    ldir = _cast(rs.light_dir / np.linalg.norm(rs.light_dir), T)
    amb, hdif, ldif = _cast(rs.headlight_ambient, T), _cast(rs.headlight_diffuse, T), _cast(rs.light_diffuse, T)
    checker = np.zeros((H, W), dtype=bool)
    for g in range(len(rs.shape)):
        m = hit & (hit_g == g)
        if not m.any():
            continue
        Rg, pg = fr[int(rs.link[g])]
        R, p = Rg @ r_rot[g].reshape(3, 3), Rg @ r_pos[g] + pg
        nw = hit_n @ R.T
        with np.errstate(divide="ignore", invalid="ignore"):
            nn = T(1) / np.sqrt((nw * nw).sum(-1))
            kv = np.maximum(-(nw * d).sum(-1) * nn * inv_len, T(0))
            kl = np.maximum(-(nw @ ldir) * nn, T(0))
        base = np.broadcast_to(r_col[g][:3], (H, W, 3))
        if rs.colour[g][7] != 0:
            hp = (cp + best[..., None] * d - p) @ R
            second = ((np.floor(hp[..., 0] / r_col[g][6]).astype(np.int64) + np.floor(hp[..., 1] / r_col[g][6]).astype(np.int64)) & 1) != 0
            base = np.where(second[..., None], r_col[g][3:6], r_col[g][:3])
            checker |= m & second
        shaded = base * (amb + hdif * kv[..., None] + ldif * kl[..., None])
        out = np.where(m[..., None], shaded, out)
    _is(T, out)
    rgb = (np.clip(out, T(0), T(1)) * T(255) + T(0.5)).astype(np.uint8)
    return rgb, checker
