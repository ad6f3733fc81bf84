"""fp64 numpy reference of include/nbx_diag.h: mass, kinetic and potential energy, momentum and mass moment of a state.

The values are taken as libnbx stores them: positions and velocities as given (fp32 or fp64), G*m rounded as nbx_upload
rounds it (G = 6.67259e-11f times m in the state's precision), eps^2 = 1e-3f widened, the per-body m |v|^2 term evaluated in
the state's precision with the reference's association (as the step kernels do).  Everything after that is fp64.  The
potential is a direct all-pairs sum over j != i, in row chunks so that n = 262144 fits in memory.
"""
import numpy as np

G32 = np.float32(6.67259e-11)
EPS2 = float(np.float32(1e-3))


def gm_as_uploaded(mass):
    m = np.asarray(mass)
    if m.dtype == np.float32:
        return (G32 * m).astype(np.float64)  # fp32 product, as upload_t<float>
    return np.float64(G32) * m.astype(np.float64)  # (double)G * m; the x1/8 prescale of the fp64 records is exact


def potential(pos, mass, i_begin=0, i_count=None, chunk=1024):
    """-1/2 sum_{i in [i_begin, i_begin + i_count)} m_i sum_{j != i} G m_j / sqrt(|x_j - x_i|^2 + eps^2), in fp64."""
    x, y, z = (np.asarray(a).astype(np.float64) for a in pos)
    m = np.asarray(mass).astype(np.float64)
    gm = gm_as_uploaded(mass)
    n = len(m)
    i_count = n - i_begin if i_count is None else i_count
    total = 0.0
    for a in range(i_begin, i_begin + i_count, chunk):
        b = min(a + chunk, i_begin + i_count)
        dx = x[None, :] - x[a:b, None]
        dy = y[None, :] - y[a:b, None]
        dz = z[None, :] - z[a:b, None]
        inv = 1.0 / np.sqrt(dx * dx + dy * dy + dz * dz + EPS2)
        inv[np.arange(b - a), np.arange(a, b)] = 0.0  # j == i excluded
        total += float(np.dot(m[a:b], inv @ gm))
    return -0.5 * total


def diagnostics(state, i_begin=0, i_count=None, potential_too=True):
    """dict with the fields of nbx_diag_t (plus etotal) for the bodies [i_begin, i_begin + i_count) of `state`
    (the dict of seven arrays nbx.initial_conditions / Context.download use; pos_* of every body)."""
    n = len(state["mass"])
    i_count = n - i_begin if i_count is None else i_count
    sl = slice(i_begin, i_begin + i_count)
    mt = np.asarray(state["mass"])[sl]
    vx, vy, vz = (np.asarray(state[k])[sl] for k in ("vel_x", "vel_y", "vel_z"))
    v2 = (vx * vx + vy * vy) + vz * vz  # in the state's precision, as euler_update
    m = mt.astype(np.float64)
    out = {
        "mass": float(m.sum()),
        "kenergy": 0.5 * float((mt * v2).astype(np.float64).sum()),
        "momentum": [float((m * v.astype(np.float64)).sum()) for v in (vx, vy, vz)],
        "mass_moment": [float((m * np.asarray(state[k])[sl].astype(np.float64)).sum()) for k in ("pos_x", "pos_y", "pos_z")],
        "i_count": i_count,
    }
    if potential_too:
        out["potential"] = potential((state["pos_x"], state["pos_y"], state["pos_z"]), state["mass"], i_begin, i_count)
        out["etotal"] = out["kenergy"] + out["potential"]
    return out


def momentum_scale(state):
    """sum m |v|: the yardstick momentum errors are judged against (the total itself nearly cancels)."""
    m = np.asarray(state["mass"]).astype(np.float64)
    v = np.sqrt(sum(np.asarray(state[k]).astype(np.float64) ** 2 for k in ("vel_x", "vel_y", "vel_z")))
    return float((m * v).sum())
