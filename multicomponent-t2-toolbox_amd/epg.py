"""Drop-ins for epg/epg.py: the EPG dictionary is built on the device (one wavefront per
(T2, flip angle)) and returned in the reference's layout.  Beyond the reference: slice profiles for 2-D multi-slice
acquisitions (slice_profile and the pulse helpers below, numpy only; the dictionary itself is the device's)."""
import numpy as np

from .plan import Met2Plan


def create_Dic_3D(Npc, T2s, T1s, nEchoes, tau, alpha_values, TR, slice_profile=None):
    """epg/epg.py:155-162 -> Dic_3D[nEchoes, Npc, len(alpha_values)]; slice_profile as for Met2Plan.build_dictionary_epg"""
    alpha_values = np.atleast_1d(np.asarray(alpha_values, dtype=np.float64))
    plan = Met2Plan(int(nEchoes), int(Npc), alpha_values.shape[0])
    try:
        plan.build_dictionary_epg(T2s, T1s, tau, alpha_values, TR, slice_profile=slice_profile)
        return plan.get_dictionary()
    finally:
        plan.close()


def create_met2_design_matrix_epg(Npc, T2s, T1s, nEchoes, tau, flip_angle, TR, slice_profile=None):
    """epg/epg.py:47-62 -> design_matrix[nEchoes, Npc]"""
    return create_Dic_3D(Npc, T2s, T1s, nEchoes, tau, [flip_angle], TR, slice_profile)[:, :, 0]


# ---- slice profiles (Lebel & Wilman, Magn Reson Med 64:1005-1014, 2010): in 2-D multi-slice multi-echo spin echo the excitation and
# refocusing angles vary across the slice and the measured decay is the integral of the echo trains over the profile
MAX_PROFILE_POINTS = 64        # met2_plan_build_dictionary_epg_profile's limit


def check_profile(r_exc, r_ref, w):
    """The three arrays of a slice profile as float64 copies, or ValueError: one length from 1 to 64, every value finite and >= 0, the
    weights not all zero (what met2_plan_build_dictionary_epg_profile accepts)."""
    r_exc, r_ref, w = (np.atleast_1d(np.array(a, dtype=np.float64)) for a in (r_exc, r_ref, w))
    n_z = r_exc.shape[0]
    if r_exc.ndim != 1 or r_ref.shape != r_exc.shape or w.shape != r_exc.shape:
        raise ValueError("slice profile: r_exc, r_ref and w must be 1-D arrays of one length")
    if not 1 <= n_z <= MAX_PROFILE_POINTS:
        raise ValueError("slice profile: 1 to %d points, got %d" % (MAX_PROFILE_POINTS, n_z))
    for name, a in (("r_exc", r_exc), ("r_ref", r_ref), ("w", w)):
        if not np.all(np.isfinite(a)) or np.any(a < 0):
            raise ValueError("slice profile: %s must be finite and >= 0" % name)
    if not w.sum() > 0:
        raise ValueError("slice profile: the weights are all zero")
    return {"r_exc": r_exc, "r_ref": r_ref, "w": w}


def slice_profile(r_exc, r_ref, w=None):
    """The profile dict {'r_exc', 'r_ref', 'w'} of build_dictionary_epg / recon_met2_arrays(slice_profile=...): r_exc[z] and r_ref[z] are
    the excitation and refocusing angles at position z relative to the nominal ones (1.0 at the centre of ideal pulses), w[z] the
    quadrature weights -- None: the trapezoid rule on a uniform grid.  1 to 64 points, every value finite and >= 0; the weights come back
    normalised to sum 1."""
    if w is None:
        w = np.ones(np.size(r_exc))
        if w.shape[0] > 1:
            w[0] = w[-1] = 0.5
    prof = check_profile(r_exc, r_ref, w)
    prof["w"] = prof["w"] / prof["w"].sum()
    return prof


def same_profile(a, b):
    """Whether two profile dicts (or None) describe the same dictionary."""
    if a is None or b is None:
        return a is None and b is None
    return all(np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)) for k in ("r_exc", "r_ref", "w"))


def hann_sinc(n, tbw):
    """RF waveform of n samples: a sinc of time-bandwidth product tbw under a Hann window (sample centres, arbitrary units)."""
    t = (np.arange(int(n)) + 0.5) / int(n) - 0.5
    return np.sinc(float(tbw) * t) * (0.5 + 0.5 * np.cos(2.0 * np.pi * t))


def pulse_profile(rf, flip_deg, tbw, z, kind):
    """Relative flip angle across the slice of the pulse `rf` (real samples) by a hard-pulse spinor simulation: sample i rotates by
    theta_i = flip_deg pi/180 rf_i / sum(rf) about x, and a spin at z (in nominal slice thicknesses, the bandwidth being tbw over the
    pulse's duration) precesses by phi = 2 pi tbw z / N about z per sample, applied as half precession, RF, half precession.
    kind names what the angle is read as and selects nothing numerically: 'excitation' is the tip angle of Mz, arccos(|alpha|^2 - |beta|^2),
    'refocusing' the angle of the crushed spin echo's efficiency |beta|^2 = sin^2(theta_eff / 2), 2 asin(min(1, |beta|)) (Pauly et al., IEEE
    Trans Med Imaging 10:53-65, 1991) -- for a unitary spinor the same angle, 2 atan2(|beta|, |alpha|), which is what is returned, over flip.
    The argument is kept so that a call says which pulse it describes; anything but the two names is a ValueError."""
    if kind not in ("excitation", "refocusing"):
        raise ValueError("kind must be 'excitation' or 'refocusing'")
    rf = np.asarray(rf, dtype=np.float64).reshape(-1)
    flip = float(flip_deg) * np.pi / 180.0
    if not flip > 0 or not rf.sum() != 0:
        raise ValueError("pulse_profile needs flip_deg > 0 and a waveform with a non-zero sum")
    z = np.asarray(z, dtype=np.float64)
    theta = flip * rf / rf.sum()
    phi = 2.0 * np.pi * float(tbw) * z / rf.shape[0]
    ph = np.exp(-0.25j * phi)                              # half a sample's precession: alpha -> alpha e^{-i phi/4}, beta -> beta e^{+i phi/4}
    al = np.ones(z.shape, dtype=np.complex128)
    be = np.zeros(z.shape, dtype=np.complex128)
    for th in theta:
        al, be = al * ph, be * np.conj(ph)
        c, s = np.cos(0.5 * th), -1j * np.sin(0.5 * th)   # rotation about x: alpha = cos(th/2), beta = -i sin(th/2)
        al, be = c * al - np.conj(s) * be, s * al + c * be
        al, be = al * ph, be * np.conj(ph)
    # |alpha|^2 + |beta|^2 = 1, so both angles are 2 atan2(|beta|, |alpha|); in that form they keep full precision at 180 degrees, where
    # arccos and asin lose half of it
    return 2.0 * np.arctan2(np.abs(be), np.abs(al)) / flip


def pulse_pair_profile(rf_exc, rf_ref, tbw_exc, tbw_ref, n_z=31, z_max=1.5, thickness_ratio=1.0, flip_exc=90.0, flip_ref=180.0):
    """slice_profile() of an excitation / refocusing pulse pair on the half profile z = 0 .. z_max (n_z points, in excitation slice
    thicknesses; the profiles are symmetric, so half of it with trapezoid weights stands for the whole).  thickness_ratio: refocusing over
    excitation slice thickness."""
    z = np.linspace(0.0, float(z_max), int(n_z))
    return slice_profile(pulse_profile(rf_exc, flip_exc, tbw_exc, z, "excitation"),
                         pulse_profile(rf_ref, flip_ref, tbw_ref, z / float(thickness_ratio), "refocusing"))
