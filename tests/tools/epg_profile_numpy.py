"""The slice-profile dictionary of met2_plan_build_dictionary_epg_profile, restated as the loop of its definition (include/met2_hip.h) over
the CPU oracle's epg_signal, which takes the refocusing and the excitation angle separately.  The reference of tests/test_gpu_epg_profile.py."""
import math

import numpy as np

from oracle import oracle


def trains(T2s, T1s, nEchoes, tau, alpha_values, r_exc, r_ref):
    """H[z][fa][e][j]: echo e of the train at alpha = (a * r_ref[z]) * pi/180, alpha_exc = ((a / 2.0) * r_exc[z]) * pi/180."""
    T2s = np.asarray(T2s, dtype=np.float64); T1s = np.asarray(T1s, dtype=np.float64)
    al = np.atleast_1d(np.asarray(alpha_values, dtype=np.float64))
    r_exc = np.atleast_1d(np.asarray(r_exc, dtype=np.float64)); r_ref = np.atleast_1d(np.asarray(r_ref, dtype=np.float64))
    rad = np.pi / 180.0
    H = np.zeros((r_exc.shape[0], al.shape[0], int(nEchoes), T2s.shape[0]))
    for z in range(r_exc.shape[0]):
        for f, a in enumerate(al):
            H[z, f] = oracle.epg_signal(int(nEchoes), float(tau), 1.0 / T1s, 1.0 / T2s, (a * r_ref[z]) * rad, ((a / 2.0) * r_exc[z]) * rad)
    return H


def dictionary_fa_major(Npc, T2s, T1s, nEchoes, tau, alpha_values, TR, r_exc, r_ref, w, want_scale=False):
    """D[fa][e][j] = acc * (1 - exp(-TR / T1s[j])), acc = sum over z ascending of w[z] * H_z[e] (product and sum rounded separately).
    want_scale: also S[fa][j] = (1 - exp(-TR / T1s[j])) * sum_z w[z] max_e |H_z[e]|, the size the parity bound is relative to."""
    T1s = np.asarray(T1s, dtype=np.float64)
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    H = trains(T2s, T1s, nEchoes, tau, alpha_values, r_exc, r_ref)
    assert H.shape[3] == int(Npc) and w.shape[0] == H.shape[0]
    acc = np.zeros(H.shape[1:])
    for z in range(w.shape[0]):
        acc = acc + (w[z] * H[z])
    scale = np.array([1.0 - math.exp(-float(TR) / t) for t in T1s])       # libm's exp, as the CPU code has it (numpy's own may differ in the last bit)
    D = acc * scale
    if not want_scale:
        return D
    S = scale * np.einsum("z,zfj->fj", w, np.max(np.abs(H), axis=2))
    return D, S


def create_Dic_3D(Npc, T2s, T1s, nEchoes, tau, alpha_values, TR, r_exc, r_ref, w):
    """Reference layout [nEchoes, Npc, nFA]."""
    return np.ascontiguousarray(np.transpose(dictionary_fa_major(Npc, T2s, T1s, nEchoes, tau, alpha_values, TR, r_exc, r_ref, w), (1, 2, 0)))
