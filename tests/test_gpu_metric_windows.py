"""The metric windows (metric_lanes / write_metrics in fit_kernel.hpp, the standalone metrics_kernel) away from the default cuts.

motor:222-224 builds the windows as  myelin: T2 <= cut_m,  intra/extra: cut_m < T2 <= cut_ie,  free water: T2 >= cut_ie  -- a bin
exactly at cut_ie belongs to the last two -- and motor:443-472 sums the normalised spectrum over them.  The reference here is those
few lines in np.longdouble.  The CPU oracle is compared with it first (no GPU needed), then the standalone metrics entry and the maps
a fit writes; the fit's maps must equal the standalone kernel's bit for bit on the fit's own spectra.

Bound: 1e-12 relative on every map.  The sums have at most 128 non-negative terms (<= 128 eps = 3e-14 relative), the exponent of
T2_M / T2_IE carries that times |log T2| <= 8: a factor of 4 in hand.  Which windows a single bin falls into is exact and compared
exactly.
"""
import importlib

import numpy as np
import pytest

PKG = "multicomponent-t2-toolbox_amd"
MAPS = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC")
EPS = 1.0e-16                                      # motor's epsilon
RTOL = 1e-12
# n_t2 -> an n_te the fit tests already run with it: one and two bins per lane, partial last lanes
SHAPES = {12: 8, 60: 32, 64: 32, 65: 32, 128: 63}


def t2_grid(n):
    return np.logspace(np.log10(10.0), np.log10(2000.0), n)       # motor:220


def cut_pairs(T2s):
    """(name, t2_myelin_cut, t2_ie_cut)"""
    n = len(T2s)
    km, kie = n // 4, (2 * n) // 3                                  # grid points inside the range, km < kie
    return [("default", 40.0, 200.0),
            ("myelin25", 25.0, 200.0),
            ("myelin-on-grid", float(T2s[km]), 200.0),
            ("ie-on-grid", 40.0, float(T2s[kie])),
            ("both-on-grid", float(T2s[km]), float(T2s[kie])),
            ("first-bin-is-the-myelin-cut", float(T2s[0]), 200.0),
            ("last-bin-is-the-ie-cut", 40.0, float(T2s[-1])),
            ("empty-myelin", 5.0, 200.0),                           # below T2s[0] = 10: MWF = 0, T2_M = exp(0) = 1
            ("empty-csf", 40.0, 3000.0),                            # above T2s[-1]
            ("empty-ie", float(T2s[km]), float(T2s[km])),           # the two cuts on one grid value: that bin is myelin AND free water
            ("empty-ie-off-grid", 60.0, 60.0)]


def windows(T2s, cut_m, cut_ie):
    return T2s <= cut_m, (T2s > cut_m) & (T2s <= cut_ie), T2s >= cut_ie          # motor:222-224


def ref_metrics(fsol, T2s, mask, cut_m, cut_ie):
    """motor:443-472 in np.longdouble -> [6, nvox] (longdouble)"""
    ld = np.longdouble
    ind_m, ind_t, ind_csf = windows(T2s, cut_m, cut_ie)
    x = np.asarray(fsol, dtype=np.float64).astype(ld)
    logT2 = np.log(T2s.astype(ld))
    vt = x.sum(axis=1) + ld(EPS)
    xn = x / vt[:, None]
    fm, fie, fcsf = xn[:, ind_m].sum(axis=1), xn[:, ind_t].sum(axis=1), xn[:, ind_csf].sum(axis=1)
    t2m = np.exp((xn[:, ind_m] * logT2[ind_m]).sum(axis=1) / (fm + ld(EPS)))
    t2ie = np.exp((xn[:, ind_t] * logT2[ind_t]).sum(axis=1) / (fie + ld(EPS)))
    out = np.stack([fm, fie, fcsf, t2m, t2ie, vt])
    out[:, np.asarray(mask) <= 0] = 0                                # motor:447: the maps stay at their initial zeros
    return out


def spectra(n, seed):
    """(fsol [nvox, n], mask [nvox], x of the one-hot rows [n]): rows 0..n-1 one-hot in bin 0..n-1, then an all-zero row, then random
    non-negative sparse spectra at scale 1, 1e-200 and 1e+200; every seventh row masked out, one-hot rows never."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(0.1, 10.0, n)                                   # below 0.5 the 1e-16 in x / (x + 1e-16) is above half an ulp of x
    x1[::3] = rng.uniform(0.1, 0.4, len(x1[::3]))
    rnd = rng.uniform(0.0, 1.0, (40, n)) * (rng.uniform(size=(40, n)) < 0.4)
    rnd[0] = rng.uniform(0.0, 1.0, n)                                # one dense row
    fsol = np.concatenate([np.diag(x1), np.zeros((1, n)), rnd, rnd * 1e-200, rnd * 1e+200])
    mask = np.ones(fsol.shape[0])
    mask[n + 3::7] = 0
    assert mask[n] == 1 and (mask == 0).sum() >= 10
    return fsol, mask, x1


def check_maps(got, fsol, T2s, mask, cut_m, cut_ie, what):
    got = np.asarray(got, dtype=np.float64)
    ref = ref_metrics(fsol, T2s, mask, cut_m, cut_ie)
    assert got.shape == ref.shape
    assert not got[:, np.asarray(mask) <= 0].any(), what              # mask == 0: zeros in all six maps
    refd = ref.astype(np.float64)
    for i, name in enumerate(MAPS):
        zero = refd[i] == 0
        assert not got[i][zero].any(), (what, name)
        err = np.abs(got[i].astype(np.longdouble) - ref[i])[~zero] / np.abs(ref[i][~zero])
        assert err.size == 0 or float(err.max()) <= RTOL, (what, name, float(err.max()))
    return refd


def check_one_hot(got, x1, T2s, cut_m, cut_ie, what):
    """rows 0..n-1 of spectra(): bin j alone, so a fraction is x / (x + 1e-16) when the bin is in that window and exactly 0 when not"""
    got = np.asarray(got, dtype=np.float64)
    n = len(T2s)
    f = x1 / (x1 + EPS)
    for i, ind in enumerate(windows(T2s, cut_m, cut_ie)):
        g = got[i, :n]
        assert np.array_equal(g != 0, ind), (what, MAPS[i], np.nonzero((g != 0) != ind)[0])
        assert np.all(np.abs(g[ind] - f[ind]) <= np.spacing(f[ind])), (what, MAPS[i])
    if cut_m < cut_ie:                                                 # a bin at cut_ie: intra/extra AND free water
        at = np.nonzero(T2s == cut_ie)[0]
        assert np.all(got[1, at] != 0) and np.all(got[2, at] != 0) and np.all(got[0, at] == 0), what


def check_empty_windows(got, name, mask):
    on = np.asarray(mask) > 0
    if name == "empty-myelin":
        assert np.all(got[0] == 0) and np.all(got[3][on] == 1.0)
    if name == "empty-csf":
        assert np.all(got[2] == 0)
    if name.startswith("empty-ie"):
        assert np.all(got[1] == 0) and np.all(got[4][on] == 1.0)


def test_cut_pairs_are_what_they_say():
    for n in SHAPES:
        T2s = t2_grid(n)
        for name, cm, cie in cut_pairs(T2s):
            m, t, c = windows(T2s, cm, cie)
            assert m.any() != (name == "empty-myelin") and c.any() != (name == "empty-csf") and t.any() != name.startswith("empty-ie"), (n, name)
            if "on-grid" in name or name == "empty-ie":
                assert (T2s == cm).any() or (T2s == cie).any()
        assert (T2s[0] == 10.0) and T2s[-1] > 2000.0 - 1e-9


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_oracle_metrics_against_numpy_windows(oracle, n):
    T2s = t2_grid(n)
    fsol, mask, x1 = spectra(n, 100 + n)
    for name, cm, cie in cut_pairs(T2s):
        m = oracle.metrics(fsol, T2s, mask, cm, cie)
        got = np.stack([m[k] for k in MAPS])
        what = ("oracle", n, name)
        check_maps(got, fsol, T2s, mask, cm, cie, what)
        check_one_hot(got, x1, T2s, cm, cie, what)
        check_empty_windows(got, name, mask)
        z = got[:, n]                                                  # the all-zero spectrum: TWC = 1e-16, T2 maps = exp(0) = 1
        assert list(z) == [0.0, 0.0, 0.0, 1.0, 1.0, EPS]


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    return importlib.import_module(PKG)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_standalone_metrics_windows(pkg, n):
    import torch
    T2s = t2_grid(n)
    fsol, mask, x1 = spectra(n, 100 + n)
    plan = pkg.Met2Plan(SHAPES[n], n, 1)
    plan.set_t2_grid(T2s)
    fs_d = torch.as_tensor(fsol, device="cuda"); mk_d = torch.as_tensor(mask, device="cuda")
    for name, cm, cie in cut_pairs(T2s):
        if name != "default":                                          # the default pair is what a new plan has
            plan.set_options(t2_myelin_cut=cm, t2_ie_cut=cie)
        assert plan.get_options("t2_myelin_cut", "t2_ie_cut") == {"t2_myelin_cut": cm, "t2_ie_cut": cie}
        got = plan.metrics(fs_d, mk_d).cpu().numpy()
        what = ("standalone", n, name)
        check_maps(got, fsol, T2s, mask, cm, cie, what)
        check_one_hot(got, x1, T2s, cm, cie, what)
        check_empty_windows(got, name, mask)
        assert list(got[:, n]) == [0.0, 0.0, 0.0, 1.0, 1.0, EPS]
        nomask = plan.metrics(fs_d).cpu().numpy()                      # no mask: every row counts
        check_maps(nomask, fsol, T2s, np.ones_like(mask), cm, cie, what + ("nomask",))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("meth", ["NNLS", "X2"])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_fit_maps_windows(pkg, n, meth):
    import torch
    synth = importlib.import_module(PKG + ".synth")
    nte, nvox = SHAPES[n], 200
    T2s = t2_grid(n)
    plan = pkg.Met2Plan(nte, n, 1)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(n), 10.0, np.array([150.0]), 3000.0).set_penalty("L2", T2s)
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=7000 + n, device="cuda")
    data[11] = 0.0                                                     # gated out (motor:115-117): an all-zero spectrum under mask > 0
    mask = torch.ones(nvox, dtype=torch.uint8, device="cuda")
    mask[5::9] = 0
    mk = mask.cpu().numpy().astype(float)
    for name, cm, cie in cut_pairs(T2s):
        if name != "default":
            plan.set_options(t2_myelin_cut=cm, t2_ie_cut=cie)
        out = plan.fit(meth, data, mask=mask)
        fsol = out["fsol"]; maps = out["maps"].cpu().numpy()
        assert (fsol[mask == 0] == 0).all() and (fsol[11] == 0).all() and (fsol.sum(dim=1) > 0).sum() >= nvox - 24
        alone = plan.metrics(fsol, mask).cpu().numpy()
        assert np.array_equal(maps, alone), (n, meth, name, np.argwhere(maps != alone)[:5])      # the fused epilogue is the standalone kernel
        what = ("fit " + meth, n, name)
        check_maps(maps, fsol.cpu().numpy(), T2s, mk, cm, cie, what)
        check_empty_windows(maps, name, mk)
        assert list(maps[:, 11]) == [0.0, 0.0, 0.0, 1.0, 1.0, EPS]
    plan.close()
