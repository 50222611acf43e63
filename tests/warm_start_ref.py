"""A numpy restatement of spdm_policy_warm_start (csrc/policy.hip), written from its description in include/spdm.h alone: the
previous plan shifted by the pushes since, re-centred on the new window's first entry, noised to an intermediate level of the
schedule and in-painted.  numpy rounds each float32 array operation on its own, so these are the kernel's bits -- except for
the drawn noise, whose logf / sinf / cosf differ between libraries (tests/test_gpu_forward_process.py derives the bound).  Test
support only."""
import numpy as np

import forward_process_ref

PURPOSE = 8          # 0 the sampler, 1-3 spdm_train_forward_process, 4-7 spdm_obs_noise

F2 = np.float32(2.0)


def rows(H, delta, step_size):
    """``(r0, r1, f)``: the rows of the old plan that row r of the new one lies between, and delta % step_size."""
    q, f = divmod(int(delta), int(step_size))
    r = np.arange(H, dtype=np.int64)
    return np.minimum(r + q, H - 1), np.minimum(r + q + (1 if f > 0 else 0), H - 1), f


def shift(prev, delta, step_size):
    """Steps 1 and 2: ``prev`` (E, H, D) float32 at the rows a plan made ``delta`` pushes later wants."""
    assert prev.dtype == np.float32 and prev.ndim == 3
    r0, r1, f = rows(prev.shape[1], delta, step_size)
    a, b = prev[:, r0, :], prev[:, r1, :]
    if f == 0:
        return a.copy()                                  # no arithmetic: every bit pattern passes through
    w = np.float32(f) / np.float32(step_size)
    g = a + w * (b - a)
    assert g.dtype == np.float32
    return g


def recentre(g, T0, T1):
    """Step 3 on the position columns of ``g`` (E, H, D): (((2 g) + T0) - T1) / 2 in float32; the other columns keep g."""
    assert g.dtype == T0.dtype == T1.dtype == np.float32
    out = g.copy()
    out[:, :, :2] = (((F2 * g[:, :, :2]) + T0[:, None, :]) - T1[:, None, :]) / F2
    return out


def guess(prev, T0, T1, delta, step_size):
    return recentre(shift(prev, delta, step_size), T0, T1)


def draw(seed, draw_index, env_offset, E, H, D):
    """Step 4: (E, H, D) float32 normals, counter (k, (uint32)(env_offset + e), draw, 8)."""
    z = forward_process_ref.draw_noise(seed, step=draw_index, sample_offset=env_offset, batch=E, elems=H * D, purpose=PURPOSE)
    return z.reshape(E, H, D)


def add_noise(g, z, sa, sb):
    """Step 5: (sa g) + (sb z), three float32 roundings."""
    x = np.float32(sa) * g + np.float32(sb) * z
    assert x.dtype == np.float32
    return x


def constrain(x, inpaint):
    """Step 6: rows r < inp_h of x are ``inpaint``'s (E, inp_h, D); None for inp_h == 0."""
    x = x.copy()
    if inpaint is not None and inpaint.shape[1] > 0:
        x[:, :inpaint.shape[1], :] = inpaint
    return x


def warm_start(prev, T0, T1, inpaint, delta, step_size, sa, sb, seed=0, env_offset=0, draw_index=0, noise=None):
    """``(x, guess, noise)``, each (E, H, D) float32."""
    E, H, D = prev.shape
    g = guess(prev, T0, T1, delta, step_size)
    z = draw(seed, draw_index, env_offset, E, H, D) if noise is None else noise
    return constrain(add_noise(g, z, sa, sb), inpaint), g, z
