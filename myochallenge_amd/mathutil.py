"""Small numpy helpers shared by the host-side model tools (quaternions are w,x,y,z), and the two torch functions that move between
qpos and its tangent space (integrate_pos / differentiate_pos: BaodingVecEnv.linearize)."""
import numpy as np


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([
        [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z],
    ])


def quat_mul(a, b):
    return np.array([
        a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
        a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
        a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
        a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0],
    ])


def axis_angle_quat(axis, angle):
    axis = np.asarray(axis, float)
    n = np.linalg.norm(axis)
    if n < 1e-300:
        return np.array([1.0, 0, 0, 0])
    s = np.sin(angle / 2) / n
    return np.array([np.cos(angle / 2), axis[0] * s, axis[1] * s, axis[2] * s])


def mat_to_quat(R):
    """Rotation matrix -> unit quaternion (w,x,y,z)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


# ---- qpos <-> tangent space, torch, any leading dimensions (MuJoCo's mj_integratePos / mj_differentiatePos with dt = 1).
# jnt_type: 0 free, 1 ball, 2 slide, 3 hinge; jnt_qposadr / jnt_dofadr: the joints' first qpos entry / dof.
def _tquat_mul(a, b):
    import torch
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _tquat_integrate(q, w):
    """q rotated by the LOCAL-frame rotation vector w (mju_quatIntegrate with dt = 1), normalised"""
    import torch
    ang = w.norm(dim=-1, keepdim=True)
    axis = w / torch.where(ang > 0, ang, torch.ones_like(ang))
    out = _tquat_mul(q, torch.cat([torch.cos(ang / 2), axis * torch.sin(ang / 2)], -1))
    out = torch.where(ang > 0, out, q)
    return out / out.norm(dim=-1, keepdim=True)


def _tquat_sub(qb, qa):
    """the local-frame rotation vector that takes qa to qb (mju_subQuat): angle in (-pi, pi]"""
    import torch
    d = _tquat_mul(torch.cat([qa[..., :1], -qa[..., 1:]], -1), qb)
    s = d[..., 1:].norm(dim=-1, keepdim=True)
    axis = d[..., 1:] / torch.where(s > 0, s, torch.ones_like(s))
    ang = 2 * torch.atan2(s, d[..., :1])
    ang = torch.where(ang > np.pi, ang - 2 * np.pi, ang)
    return axis * ang


def integrate_pos(qpos, dq, jnt_type, jnt_qposadr, jnt_dofadr):
    """qpos [..., nq] moved by the tangent vector dq [..., nv]: hinge and slide entries add; a free joint's position adds and its
    quaternion is rotated by the local-frame rotation vector (a ball joint's likewise); the quaternions come out normalised"""
    import torch
    out = qpos.clone()
    for ty, qa, da in zip(jnt_type, jnt_qposadr, jnt_dofadr):
        ty, qa, da = int(ty), int(qa), int(da)
        if ty == 0:
            out[..., qa:qa + 3] = qpos[..., qa:qa + 3] + dq[..., da:da + 3]
            out[..., qa + 3:qa + 7] = _tquat_integrate(qpos[..., qa + 3:qa + 7], dq[..., da + 3:da + 6])
        elif ty == 1:
            out[..., qa:qa + 4] = _tquat_integrate(qpos[..., qa:qa + 4], dq[..., da:da + 3])
        else:
            out[..., qa] = qpos[..., qa] + dq[..., da]
    return out


def differentiate_pos(q1, q0, jnt_type, jnt_qposadr, jnt_dofadr):
    """the tangent vector [..., nv] that takes q0 to q1 (both [..., nq]): integrate_pos(q0, differentiate_pos(q1, q0)) == q1"""
    import torch
    nv = max(int(da) + (6 if int(ty) == 0 else 3 if int(ty) == 1 else 1) for ty, da in zip(jnt_type, jnt_dofadr)) if len(jnt_type) else 0
    out = torch.zeros(q1.shape[:-1] + (nv,), dtype=q1.dtype, device=q1.device)
    for ty, qa, da in zip(jnt_type, jnt_qposadr, jnt_dofadr):
        ty, qa, da = int(ty), int(qa), int(da)
        if ty == 0:
            out[..., da:da + 3] = q1[..., qa:qa + 3] - q0[..., qa:qa + 3]
            out[..., da + 3:da + 6] = _tquat_sub(q1[..., qa + 3:qa + 7], q0[..., qa + 3:qa + 7])
        elif ty == 1:
            out[..., da:da + 3] = _tquat_sub(q1[..., qa:qa + 4], q0[..., qa:qa + 4])
        else:
            out[..., da] = q1[..., qa] - q0[..., qa]
    return out
