"""``aft_lmmse_f32``, ``hip_ops.LmmsePlan`` and ``lmmse.LmmseEstimator`` on the HIP device: the kernel against the float64 definition
within a bound DERIVED here from the tables and the frame's pilots, batch independence bit for bit, condition arrays in pinned host
memory, no unwritten output, the checked build, the module and the evaluation sweep without a synchronisation, the entry point's refusals.

The bound (``derived_bound``).  u = 2^-24 is float32's unit roundoff, gamma(n) = n u / (1 - n u).  The device reads the float32 ROUNDING
of each table entry (u relative, per real component) and the frame's complex64 pilots exactly; the comparison is against the float64
definition itself.  Every product stage of k_lmmse.hip is a sum of fused multiply-adds, so a real dot product of n terms errs by at most
gamma(n) times the dot product of the absolute values, in any order.  A complex x complex product of n terms is two real dot products
of 2n terms, each bounded through |a_r||b_r| + |a_i||b_i| <= |a||b|: sqrt(2) gamma(2n) sum |a||b| in modulus; a complex x real product
of n terms errs by gamma(n) sum |a||b| in modulus.  Writing |.| for element-wise moduli, e for the bound on a stage's error and m >= the
modulus of what the device holds:

* Y1 = U_f^H P:        e1 = ((1 + u)(1 + sqrt(2) gamma(2 Ps)) - 1) |U_f^H||P|,                     m1 = |U_f^H||P| + e1
* Y  = Y1 U_t:         e2 = e1 |U_t| + ((1 + u)(1 + gamma(Pt)) - 1) m1 |U_t|,                      m2 = |U_f^H||P||U_t| + e2
* D  = 1 / (lf lt + s2): the three inputs are rounded and all terms are non-negative, the fused multiply-add rounds once: the
  denominator is within ex = (1 + u)^3 - 1; the division is within 2.5 ulp = 5 u (the OpenCL limit the device library is built to;
  the compiler's default is the correctly rounded one):  rD = (1 + ex / (1 - ex))(1 + 5 u) - 1
* C  = D o Y (one rounding per component):  e3 = D o (((1 + rD)(1 + u) - 1) m2 + e2),              m3 = D o (|U_f^H||P||U_t|) + e3
* V  = C T'^T:         e4 = e3 |T'|^T + ((1 + u)(1 + gamma(Pt)) - 1) m3 |T'|^T,                    m4 = (m3 - e3) |T'|^T + e4
* est = F' V:          e5 = |F'| e4 + ((1 + u)(1 + sqrt(2) gamma(2 Ps)) - 1) |F'| m4
The bound is per element and per frame; it is evaluated on absolute values, so it does not see cancellation (it sits one to three orders
above what is observed).  Observed maxima are printed; DESIGN.md records them.  (A float32-subnormal eigenvalue would escape the
relative-rounding model; next to noise_var it changes D by less than 1e-30.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, make_pack, simulate_frames_host
from adafortitran_amd.hip_ops import LmmsePlan
from adafortitran_amd.lmmse import LmmseEstimator, LmmseTables, lmmse_estimate_host
from helpers import TOL_HIP_MSE
from test_chansim_gpu import _bits, _no_sync, _poison, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _gamma(n):
    return n * U / (1.0 - n * U)


def derived_bound(tb: LmmseTables, pilots: np.ndarray, idx) -> np.ndarray:
    """Bound on |device estimate - definition| per element, [n, S, T]; module docstring."""
    Ps, Pt = tb.cfg.pilot
    r2 = np.sqrt(2.0)
    cc = (1 + U) * (1 + r2 * _gamma(2 * Ps)) - 1          # complex x complex stage of Ps terms, rounded table
    cr = (1 + U) * (1 + _gamma(Pt)) - 1                   # complex x real stage of Pt terms, rounded table
    ex = (1 + U) ** 3 - 1
    r_d = (1 + ex / (1 - ex)) * (1 + 5 * U) - 1
    out = np.empty((len(pilots), *tb.cfg.ofdm))
    for n, (a, d, e) in enumerate(zip(*idx)):
        ufh, ut, tp, fp, gain = np.abs(tb.u_f[d].conj().T), np.abs(tb.u_t[e]), np.abs(tb.t[e]), np.abs(tb.f[d]), tb.gain(a, d, e)
        a1 = ufh @ np.abs(pilots[n])
        e1 = cc * a1
        m1 = a1 + e1
        a2 = a1 @ ut
        e2 = e1 @ ut + cr * (m1 @ ut)
        m2 = a2 + e2
        e3 = gain * (((1 + r_d) * (1 + U) - 1) * m2 + e2)
        m3 = gain * a2 + e3
        e4 = e3 @ tp.T + cr * (m3 @ tp.T)
        m4 = (gain * a2) @ tp.T + e4
        out[n] = fp @ e4 + cc * (fp @ m4)
    return out


_cache = {}


def _case(name):
    """(cfg, tables, plan, pilots complex64 [b,Ps,Pt], meta float32 [b,3], definition complex128 [b,S,T]), made once per configuration."""
    if name not in _cache:
        cfg, b = CONFIGS[name]
        tb = LmmseTables(cfg)
        _, pilots, meta = simulate_frames_host(cfg, 11, np.arange(b))
        pilots = pilots.astype(np.complex64)
        want = lmmse_estimate_host(tb, pilots, meta)
        for a in (pilots, meta, want):
            a.setflags(write=False)
        _cache[name] = (cfg, tb, LmmsePlan(tb, DEV), pilots, meta, want)
    return _cache[name]


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def _conds(meta, where=DEV):
    cols = [torch.from_numpy(np.array(meta[:, k])) for k in range(3)]
    return [c.pin_memory() if where == "pinned" else c.to(where) for c in cols]


CONFIGS = {
    "default_120x14": (ChannelSimConfig(), 3),
    "odd_30x7": (ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3)), 5),                   # odd T: 8-byte stores, a partial column group
    "three_tiles_24x37": (ChannelSimConfig(ofdm=(24, 37), pilot=(4, 5)), 2),         # three time tiles, a ragged last one
    "lds_bound_128x40": (ChannelSimConfig(ofdm=(128, 40), pilot=(64, 16)), 2),       # the LDS plan at its bound
    "degenerate_1x1": (ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), 1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_against_the_float64_definition(name):
    cfg, tb, plan, pilots, meta, want = _case(name)
    b = len(pilots)
    bound = derived_bound(tb, pilots, tb.indices(meta))
    _poison([((b, *cfg.ofdm), torch.complex64)])                  # an element the kernel leaves unwritten would come back NaN
    est = plan(_dev(pilots), *_conds(meta))
    assert est.shape == want.shape and est.dtype == torch.complex64 and est.is_cuda
    got = est.cpu().numpy().astype(np.complex128)
    assert np.isfinite(got).all()
    err, scale = np.abs(got - want), float(np.abs(want).max())
    print(f"{name}: max|est - def| {err.max():.3e} = {err.max() / scale:.3e} |h|max   largest err / bound {float((err / bound).max()):.3f}   "
          f"(bound up to {bound.max():.3e} = {bound.max() / scale:.3e} |h|max)")
    assert (err <= bound).all()


def test_a_frame_does_not_depend_on_its_batch_or_its_position():
    for name in ("default_120x14", "odd_30x7", "three_tiles_24x37"):
        cfg, tb, plan, pilots, meta, _ = _case(name)
        alone = plan(_dev(pilots[:1]), *_conds(meta[:1]))
        _, many_p, many_m = simulate_frames_host(cfg, 12, np.arange(37))
        many_p = many_p.astype(np.complex64)
        many_p[[4, 36]], many_m[[4, 36]] = pilots[0], meta[0]
        batch = plan(_dev(many_p), *_conds(many_m))
        _same_bits([batch[4:5], batch[36:37]], [alone, alone])
        one_by_one = torch.cat([plan(_dev(many_p[i:i + 1]), *_conds(many_m[i:i + 1])) for i in (0, 17, 35)])
        _same_bits([batch[[0, 17, 35]]], [one_by_one])


def test_conditions_in_pinned_memory_null_pointers_and_the_selection_rule():
    cfg, tb, plan, pilots, meta, _ = _case("default_120x14")
    _, p37, m37 = simulate_frames_host(cfg, 13, np.arange(37))
    p37 = p37.astype(np.complex64)
    m37[:6] = [[12.4, 120.0, 1301.0], [np.nan, 1e6, -5.0], [2.5, 75.0, 300.0], [np.inf, np.nan, np.nan], [-np.inf, 349.0, 1e5],
               [7.5, 325.0, 1100.0]]                              # off the tables: nearest value, ties to the lower index, NaN to 0
    want = plan(_dev(p37), *_conds(m37))
    got = plan(torch.from_numpy(p37).pin_memory(), *_conds(m37, "pinned"))          # every input read in place from pinned host memory
    _same_bits([got], [want])
    # the kernel's choice of design point is the host's: the frames estimated one design point at a time, pinned by index
    idx = np.stack(tb.indices(m37), axis=1)
    assert idx[:6].tolist() == [[2, 1, 6], [0, 6, 0], [0, 0, 0], [0, 0, 0], [0, 6, 6], [1, 5, 4]]
    snr, ds, dop = (np.asarray(cfg.tables()[k]) for k in ("snr_db", "delay_spread_ns", "doppler_hz"))
    for i in (0, 1, 2, 3, 4, 5, 20):
        a, d, e = idx[i]
        pinned = LmmsePlan(tb, DEV, assume=dict(snr_db=snr[a], delay_spread_ns=ds[d], doppler_hz=dop[e]))
        assert pinned.fixed == (a, d, e)
        _same_bits([pinned(_dev(p37[i:i + 1]))], [want[i:i + 1]])                    # three NULL condition pointers
    # one condition pinned: its pointer may be NULL, the other two are read
    part = LmmsePlan(tb, DEV, assume=dict(delay_spread_ns=200))
    c = _conds(m37)
    m200 = m37.copy()
    m200[:, 1] = 200.0
    _same_bits([part(_dev(p37), c[0], None, c[2])], [plan(_dev(p37), *_conds(m200))])
    _same_bits([part(_dev(p37), *c)], [plan(_dev(p37), *_conds(m200))])              # ... and is not read when it is given
    with pytest.raises(ValueError, match="ds is required"):
        plan(_dev(p37), c[0], None, c[2])
    with pytest.raises(ValueError, match="pinned host memory"):
        plan(torch.from_numpy(p37), *c)
    with pytest.raises(ValueError, match="one value per frame"):
        plan(_dev(p37), c[0][:5], c[1], c[2])
    with pytest.raises(ValueError, match="HIP device"):
        LmmsePlan(tb, "cpu")


def test_the_8_byte_store_form_on_a_base_off_16_bytes():
    """The caching allocator only hands out 512-byte aligned blocks; a base 8 bytes off goes through the entry point directly."""
    cfg, tb, plan, pilots, meta, _ = _case("default_120x14")
    b = len(pilots)
    pil, conds = _dev(pilots), _conds(meta)
    want = plan(pil, *conds)
    flat = torch.empty((b * 120 * 14 + 1,), dtype=torch.complex64, device=DEV)
    torch.view_as_real(flat).fill_(float("nan"))                  # both components: torch.full(nan) would leave the imaginary parts 0
    assert (flat.data_ptr() + 8) % 16 == 8
    _lib.check(_lib.load().aft_lmmse_f32(ctypes.byref(plan.plan), plan.image.data_ptr(), pil.data_ptr(), *(c.data_ptr() for c in conds),
                                         flat.data_ptr() + 8, b, _lib.current_stream_ptr(flat.device)))
    _same_bits([flat[1:].view(b, 120, 14)], [want])
    assert torch.isnan(torch.view_as_real(flat[:1])).all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_lmmse_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_lmmse_f32")
    for name in CONFIGS:
        cfg, tb, plan, pilots, meta, _ = _case(name)
        _same_bits([plan(_dev(pilots), *_conds(meta), lib=lib)], [plan(_dev(pilots), *_conds(meta))])
    cfg, tb, plan, pilots, meta, _ = _case("default_120x14")
    pinned = LmmsePlan(tb, DEV, assume=dict(snr_db=10, delay_spread_ns=350, doppler_hz=1400))
    _same_bits([pinned(_dev(pilots), lib=lib)], [pinned(_dev(pilots))])


def test_module_runs_from_the_loaders_without_a_synchronisation():
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to(DEV).eval()
    assert model.table_image.is_cuda and list(model.parameters()) == []
    loader = SynthLoader(cfg, 16, 16 * 5, device=DEV, seed=2)
    it = iter(loader)
    first = next(it)
    outs = [model(first[0], first[2])]                               # the first forward builds the plan and pins the ring: outside the guard
    torch.cuda.synchronize()
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                                             # the mode is honoured: what follows is not vacuous
        batches = [first] + list(it)
        outs += [model(p, m) for p, _, m in batches[1:]]
    assert len(outs) == 5
    tb = model.tables
    for (pil, ideal, meta), est in zip(batches, outs):
        assert est.is_cuda and est.shape == ideal.shape and est.dtype == torch.complex64 and not meta[1].is_cuda
        cond = np.concatenate([m.numpy() for m in meta[1:4]], axis=1)
        p = pil.cpu().numpy()
        want = lmmse_estimate_host(tb, p, cond)
        assert (np.abs(est.cpu().numpy() - want) <= derived_bound(tb, p, tb.indices(cond))).all()
    # CPU-tensor batches (ResidentLoader on the CPU) go through the pinned ring: the same bits as device-resident inputs, for more
    # batches than the ring has slots, with nothing enqueued but the launch
    pack = make_pack(cfg, 80, seed=6)
    host_batches = list(ingest.ResidentLoader(pack, cfg.pilot, 8, device="cpu", shuffle=False))
    assert len(host_batches) == 10 and not host_batches[0][0].is_cuda and not host_batches[0][0].is_pinned()
    resident = [model(p.to(DEV), tuple(m.to(DEV) if torch.is_tensor(m) else m for m in meta)) for p, _, meta in host_batches]
    torch.cuda.synchronize()
    with _no_sync():
        ringed = [model(p, meta) for p, _, meta in host_batches]
    _same_bits(ringed, resident)
    # every condition pinned: no meta needed
    fixed = LmmseEstimator(cfg, assume=dict(snr_db=10, delay_spread_ns=350, doppler_hz=1400)).to(DEV)
    p = host_batches[0][0].numpy()
    want = lmmse_estimate_host(tb, p, None, assume=fixed.assume)
    got = fixed(host_batches[0][0]).cpu().numpy()
    assert (np.abs(got - want) <= derived_bound(tb, p, tb.indices(np.zeros((len(p), 3)), fixed.assume))).all()


def test_evaluation_sweep_over_simulated_packs():
    from adafortitran_amd.evaluation import get_test_stats
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to(DEV)
    tb = model.tables
    packs = {snr: make_pack(cfg, 256, seed=20 + snr, snr_db=snr) for snr in (0, 10, 20)}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, cfg.pilot, 128, device=DEV, shuffle=False)) for snr, pack in packs.items()]
    stats = get_test_stats(model, loaders)
    assert list(stats) == [0, 10, 20]
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    for snr, pack in packs.items():
        pil = pack["h_ls_sparse"][:, sc[:, None], sym[None, :]]
        want = lmmse_estimate_host(tb, pil, pack["meta"][:, 1:4])
        mse = float((np.abs(want - pack["h_ideal"]) ** 2).mean())
        ls = float((np.abs(pack["h_ls_full"].astype(np.complex128) - pack["h_ideal"]) ** 2).mean())
        got = 10.0 ** (stats[snr] / 10.0)
        print(f"SNR {snr}: LMMSE on the device {got:.6e}  definition {mse:.6e}  |d|/MSE {abs(got - mse) / mse:.3e}   LS {ls:.4e}")
        assert abs(got - mse) <= TOL_HIP_MSE * mse
        assert got < ls


def test_every_refusal_of_the_entry_point_launches_nothing():
    cfg, tb, plan, pilots, meta, _ = _case("default_120x14")
    lib, b = _lib.load(), len(pilots)
    est = torch.empty((b, 120, 14), dtype=torch.complex64, device=DEV)
    torch.view_as_real(est).fill_(float("nan"))                   # both components: torch.full(nan) would leave the imaginary parts 0
    pil, conds = _dev(pilots), _conds(meta)
    good = dict(tables=plan.image.data_ptr(), pilots=pil.data_ptr(), snr=conds[0].data_ptr(), ds=conds[1].data_ptr(),
                dop=conds[2].data_ptr(), est=est.data_ptr(), batch=b)

    def call(p=None, **kw):
        a = dict(good, **kw)
        return lib.aft_lmmse_f32(ctypes.byref(p if p is not None else tb.to_struct()), a["tables"], a["pilots"], a["snr"], a["ds"],
                                 a["dop"], a["est"], a["batch"], None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_lmmse_f32(None, good["tables"], good["pilots"], good["snr"], good["ds"], good["dop"], good["est"], b, None)
    assert rc == E and "NULL" in lib.aft_last_error().decode()
    for k in ("tables", "pilots", "est"):
        refused(E, "NULL pointer", **{k: None})
        refused(E, "8-byte", **{k: good[k] + 4})
    for k in ("snr", "ds", "dop"):
        refused(E, "NULL condition", **{k: None})
        refused(E, "4-byte", **{k: good[k] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for field, value, word in (("num_scs", 0, "num_scs = 0"), ("num_symbols", -1, "num_symbols = -1"), ("pilot_scs", 65, "pilot_scs = 65 is outside 1..64"),
                               ("pilot_symbols", 17, "pilot_symbols = 17 is outside 1..16"), ("pilot_scs", 0, "pilot_scs = 0"),
                               ("n_snr", 17, "n_snr = 17 is outside 1..16"), ("n_ds", 0, "n_ds = 0"), ("n_dop", 17, "n_dop = 17"),
                               ("fixed_snr", 7, "fixed_snr = 7 is outside -1..6"), ("fixed_ds", -2, "fixed_ds = -2"),
                               ("fixed_dop", 16, "fixed_dop = 16"), ("num_symbols", 1, "larger than the ofdm grid")):
        p = tb.to_struct()
        setattr(p, field, value)
        refused(SH, word, p=p)
        assert lib.aft_lmmse_table_floats(ctypes.byref(p)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(torch.view_as_real(est)).all()                                # nothing was launched
    assert lib.aft_lmmse_table_floats(ctypes.byref(tb.to_struct())) == plan.image.numel() == 7 * (2 * 144 + 2 * 12 * 120 + 12) + 7 * (4 + 28 + 2)
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(est)).all()                             # ... and the good call writes it all
    with pytest.raises(ValueError, match="table image"):
        LmmsePlan(tb, DEV, image=plan.image[:-1])
