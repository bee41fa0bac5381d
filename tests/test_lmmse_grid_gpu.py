"""``aft_lmmse_grid_f32`` and ``hip_ops.LmmseGridPlan`` on the HIP device: the kernel against the float64 definition
(``lmmse.lmmse_grid_host``) within a bound DERIVED here, batch independence bit for bit, no unwritten output, the 8-byte store form on a
base off 16 bytes, the checked build, and the refusals of the plan and of the entry point.

The observations are the float64 twin's (``linksim.link_observe_host`` on tests/test_linkdd.py's ``dd_inputs``, 16-QAM, rounded to
complex64), so both sides filter the same numbers.  The shapes: the default grid (16 frames, 16-byte stores, four chunks of rows,
Kf = 12), 30 x 7 (odd T: 8-byte stores, a ragged chunk), 3 x 5 (Kf = 3 < taps, one short chunk) and 300 x 4 (more subcarriers than
threads: ten chunks, the S-deep product at its longest here).

The bound (``derived_grid_bound``) is tests/test_lmmse_gpu.py's ``derived_bound`` with the same stages and (S, T, Kf) for the term
counts.  u = 2^-24, gamma(n) = n u / (1 - n u); the device reads the float32 rounding of each table entry (u relative per real
component) and the complex64 observations exactly; every product stage is a sum of fused multiply-adds:

* Y1 = U_g^H Z  (complex x complex, S terms):  e1 = ((1 + u)(1 + sqrt(2) gamma(2 S)) - 1) |U_g^H||Z|,      m1 = |U_g^H||Z| + e1
* Y  = Y1 U_tg  (complex x real, T terms):     e2 = e1 |U_tg| + ((1 + u)(1 + gamma(T)) - 1) m1 |U_tg|,      m2 = |U_g^H||Z||U_tg| + e2
* D  = 1 / (lg ltg + beta s2): three rounded inputs, non-negative terms, one fused multiply-add, a division within 2.5 ulp:
  rD = (1 + ex / (1 - ex))(1 + 5 u) - 1 with ex = (1 + u)^3 - 1
* C  = D o Y:   e3 = D o (((1 + rD)(1 + u) - 1) m2 + e2),                                                   m3 = D o (|U_g^H||Z||U_tg|) + e3
* V  = C T_g^T (complex x real, T terms):      e4 = e3 |T_g|^T + ((1 + u)(1 + gamma(T)) - 1) m3 |T_g|^T,    m4 = (m3 - e3) |T_g|^T + e4
* est = F_g V  (complex x complex, Kf terms):  e5 = |F_g| e4 + ((1 + u)(1 + sqrt(2) gamma(2 Kf)) - 1) |F_g| m4
It is evaluated on absolute values, so it does not see cancellation.  Observed maxima are printed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig
from adafortitran_amd.hip_ops import LmmseGridPlan
from adafortitran_amd.linksim import LinkConfig, data_noise_scale, link_observe_host
from adafortitran_amd.lmmse import LmmseTables, lmmse_grid_host
from test_chansim_gpu import _poison, _same_bits
from test_linkdd import DD_GRIDS, dd_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
M = 4
BETA = data_noise_scale(M)


def _gamma(n):
    return n * U / (1.0 - n * U)


def derived_grid_bound(tb: LmmseTables, z: np.ndarray, idx, noise_scale: float) -> np.ndarray:
    """Bound on |device estimate - definition| per element, [n, S, T]; module docstring."""
    g = tb.grid()
    S, T = tb.cfg.ofdm
    r2 = np.sqrt(2.0)
    cc_s = (1 + U) * (1 + r2 * _gamma(2 * S)) - 1
    cc_k = (1 + U) * (1 + r2 * _gamma(2 * g.kf)) - 1
    cr = (1 + U) * (1 + _gamma(T)) - 1
    ex = (1 + U) ** 3 - 1
    r_d = (1 + ex / (1 - ex)) * (1 + 5 * U) - 1
    out = np.empty(z.shape)
    for n, (a, d, e) in enumerate(zip(*idx)):
        ugh, ut = np.abs(g.u_g[d].conj().T), np.abs(g.u_tg[e])
        tp, fp, gain = np.abs(g.u_tg[e] * g.lam_tg[e][None, :]), np.abs(g.u_g[d] * g.lam_g[d][None, :]), g.gain(a, d, e, noise_scale)
        a1 = ugh @ np.abs(z[n])
        e1 = cc_s * a1
        m1 = a1 + e1
        a2 = a1 @ ut
        e2 = e1 @ ut + cr * (m1 @ ut)
        m2 = a2 + e2
        e3 = gain * (((1 + r_d) * (1 + U) - 1) * m2 + e2)
        m3 = gain * a2 + e3
        e4 = e3 @ tp.T + cr * (m3 @ tp.T)
        m4 = (gain * a2) @ tp.T + e4
        out[n] = fp @ e4 + cc_k * (fp @ m4)
    return out


_cache = {}


def _case(name):
    """(cfg, tables, plan, z complex64 [n,S,T], meta float32 [n,3], definition complex128 [n,S,T]), made once per grid."""
    if name not in _cache:
        sim, keys, sigma, _, ideal, pilots, meta, est = dd_inputs(name)
        tb = LmmseTables(sim)
        z = link_observe_host(LinkConfig(sim, M), keys, ideal, est, sigma, np.ones(len(keys), dtype=np.float32), pilots)[0]
        z = z.astype(np.complex64)
        want = lmmse_grid_host(tb, z, meta, noise_scale=BETA)
        for a in (z, want):
            a.setflags(write=False)
        _cache[name] = (sim, tb, LmmseGridPlan(tb, DEV, noise_scale=BETA), z, meta, want)
    return _cache[name]


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def nan_complex(shape) -> torch.Tensor:
    """complex64 on the device with NaN in BOTH components (``torch.full`` with a real NaN leaves the imaginary parts 0)."""
    t = torch.empty(shape, dtype=torch.complex64, device=DEV)
    torch.view_as_real(t).fill_(float("nan"))
    return t


def _conds(meta):
    return [_dev(meta[:, k]) for k in range(3)]


@pytest.mark.parametrize("name", list(DD_GRIDS))
def test_kernel_against_the_float64_definition(name):
    cfg, tb, plan, z, meta, want = _case(name)
    bound = derived_grid_bound(tb, z, tb.indices(meta), BETA)
    _poison([((len(z), *cfg.ofdm), torch.complex64)])             # an element the kernel leaves unwritten would come back NaN
    est = plan(_dev(z), *_conds(meta))
    assert est.shape == want.shape and est.dtype == torch.complex64 and est.is_cuda
    got = est.cpu().numpy().astype(np.complex128)
    assert np.isfinite(got).all()
    err, scale = np.abs(got - want), float(np.abs(want).max())
    print(f"{name}: Kf = {plan.kf}  max|est - def| {err.max():.3e} = {err.max() / scale:.3e} |h|max   largest err / bound "
          f"{float((err / bound).max()):.3f}   (bound up to {bound.max():.3e} = {bound.max() / scale:.3e} |h|max)")
    assert (err <= bound).all()


def test_pinned_conditions_need_no_arrays_and_follow_the_selection_rule():
    cfg, tb, _, z, meta, _ = _case("odd_30x7")
    pinned = dict(snr_db=21.0, delay_spread_ns=190.0, doppler_hz=900.0)      # nearest values: 20, 200, 800 (900 ties to the lower)
    plan = LmmseGridPlan(tb, DEV, assume=pinned, noise_scale=BETA)
    got = plan(_dev(z)).cpu().numpy().astype(np.complex128)
    want = lmmse_grid_host(tb, z, None, assume=pinned, noise_scale=BETA)
    fixed = np.tile(np.asarray([[20.0, 200.0, 800.0]]), (len(z), 1))
    assert (np.abs(got - want) <= derived_grid_bound(tb, z, tb.indices(fixed), BETA)).all()
    _same_bits([plan(_dev(z))], [_case("odd_30x7")[2](_dev(z), *_conds(fixed.astype(np.float32)))])


def test_a_frame_does_not_depend_on_its_batch_or_its_position():
    for name in ("default_120x14", "odd_30x7", "tall_300x4"):
        cfg, tb, plan, z, meta, _ = _case(name)
        alone = plan(_dev(z[:1]), *_conds(meta[:1]))
        idx = (np.arange(37) * 5 + 1) % len(z)
        idx[[4, 36]] = 0
        batch = plan(_dev(z[idx]), *_conds(meta[idx]))
        _same_bits([batch[4:5], batch[36:37]], [alone, alone])
        _same_bits([plan(_dev(z), *_conds(meta))[idx]], [batch])


def _entry(plan, z, conds, est_ptr, batch, lib=None, kf=None, struct=None):
    lib = lib or _lib.load()
    return lib.aft_lmmse_grid_f32(ctypes.byref(plan.plan if struct is None else struct), plan.kf if kf is None else kf, plan.image.data_ptr(),
                                  z, *conds, est_ptr, batch, _lib.current_stream_ptr(plan.image.device))


def test_the_8_byte_store_form_on_a_base_off_16_bytes_and_nothing_beside_the_output():
    for name in ("default_120x14", "odd_last_alone_3x5"):
        cfg, tb, plan, z, meta, _ = _case(name)
        zd, conds = _dev(z), _conds(meta)
        want = plan(zd, *conds)
        flat = nan_complex((want.numel() + 2,))
        assert (flat.data_ptr() + 8) % 16 == 8
        _lib.check(_entry(plan, zd.data_ptr(), [c.data_ptr() for c in conds], flat.data_ptr() + 8, len(z)))
        _same_bits([flat[1:-1]], [want.reshape(-1)])
        assert torch.view_as_real(flat[:1]).isnan().all() and torch.view_as_real(flat[-1:]).isnan().all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_lmmse_grid_f32"):       # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION
    for name in DD_GRIDS:
        cfg, tb, plan, z, meta, _ = _case(name)
        _same_bits([plan(_dev(z), *_conds(meta), lib=lib)], [plan(_dev(z), *_conds(meta))])


def test_what_the_plan_refuses():
    cfg, tb, plan, z, meta, _ = _case("odd_30x7")
    with pytest.raises(ValueError, match="at most 32"):
        LmmseGridPlan(ChannelSimConfig(ofdm=(12, 33), pilot=(2, 2)), DEV)         # T = 33
    with pytest.raises(ValueError, match="LmmseGridPlan runs on a HIP device"):
        LmmseGridPlan(tb, "cpu")
    with pytest.raises(ValueError, match="noise_scale"):
        LmmseGridPlan(tb, DEV, noise_scale=0.0)
    with pytest.raises(ValueError, match="grid image must be"):
        LmmseGridPlan(tb, DEV, image=torch.zeros(5, device=DEV))
    zd = _dev(z)
    with pytest.raises(ValueError, match="Expected observations"):
        plan(zd[:, :29], *_conds(meta))
    with pytest.raises(ValueError, match="complex64"):
        plan(zd.to(torch.complex128), *_conds(meta))
    with pytest.raises(ValueError, match="snr is required"):
        plan(zd, None, *_conds(meta)[1:])
    with pytest.raises(ValueError, match="one value per frame"):
        plan(zd, _conds(meta)[0][:3], *_conds(meta)[1:])


def test_every_refusal_of_the_entry_point_launches_nothing():
    cfg, tb, plan, z, meta, _ = _case("odd_30x7")
    lib, zd, conds = _lib.load(), _dev(z), _conds(meta)
    est = nan_complex((len(z), *cfg.ofdm))
    cp = [c.data_ptr() for c in conds]
    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE

    def refused(code, word, rc):
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    refused(E, "NULL pointer", lib.aft_lmmse_grid_f32(None, plan.kf, plan.image.data_ptr(), zd.data_ptr(), *cp, est.data_ptr(), len(z), None))
    refused(E, "NULL pointer", _entry(plan, None, cp, est.data_ptr(), len(z)))
    refused(E, "NULL pointer", _entry(plan, zd.data_ptr(), cp, None, len(z)))
    refused(E, "8-byte", _entry(plan, zd.data_ptr() + 4, cp, est.data_ptr(), len(z)))
    refused(E, "8-byte", _entry(plan, zd.data_ptr(), cp, est.data_ptr() + 4, len(z)))
    refused(E, "4-byte", _entry(plan, zd.data_ptr(), [cp[0] + 2, *cp[1:]], est.data_ptr(), len(z)))
    refused(E, "batch must be at least 1", _entry(plan, zd.data_ptr(), cp, est.data_ptr(), 0))
    refused(E, "NULL condition array", _entry(plan, zd.data_ptr(), [None, *cp[1:]], est.data_ptr(), len(z)))
    for kf in (0, -1, 31, 33):                                                    # S = 30: kf is at most min(S, 32)
        refused(SH, f"kf = {kf}", _entry(plan, zd.data_ptr(), cp, est.data_ptr(), len(z), kf=kf))
    long = LmmseTables(ChannelSimConfig(ofdm=(12, 33), pilot=(2, 2))).to_struct()  # T = 33
    refused(SH, "num_symbols = 33: the full-grid smoother filters all T symbols", _entry(plan, zd.data_ptr(), cp, est.data_ptr(), 1, kf=12, struct=long))
    bad = tb.to_struct()
    bad.n_ds = 17
    refused(SH, "n_ds = 17", _entry(plan, zd.data_ptr(), cp, est.data_ptr(), len(z), struct=bad))
    torch.cuda.synchronize()
    assert torch.view_as_real(est).isnan().all()                                  # nothing was launched
    _lib.check(_entry(plan, zd.data_ptr(), cp, est.data_ptr(), len(z)))
    _same_bits([est], [plan(zd, *conds)])                                         # ... and the good call writes it all
