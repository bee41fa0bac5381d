"""``aft_lmmse_seq_f32``, ``hip_ops.LmmseSeqPlan`` and ``lmmse.LmmseEstimator(window=, horizon=)`` on the HIP device: the kernel against
the float64 definition within a DERIVED bound, the bit identities that tie it to ``aft_lmmse_f32`` and to itself (window cut out of a
longer sequence, batch independence, pinned inputs, NULL conditions, the 8-byte store form, the checked build), no unwritten output and
no read of a slot outside the window, the module and the evaluation sweep without a synchronisation, the entry point's refusals.

The bound (``seq_bound``) is ``test_lmmse_gpu.derived_bound`` restated per frame with ``Pt -> w Pt``: the rounding model is the one of
that file's docstring (float32 roundings of the table entries, every product stage a chain of fused multiply-adds, the division within
2.5 ulp), the frame's pilot matrix is its window's ``[Ps, w Pt]``, the time tables are those of ``w``, and the two complex x real stages
have ``w Pt`` terms.  A frame without a window (``k < h``) is exact: its bound is 0 and the device's zeros must be zeros."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, make_pack, simulate_frames_host
from adafortitran_amd.hip_ops import LmmsePlan, LmmseSeqPlan
from adafortitran_amd.lmmse import LmmseEstimator, LmmseTables, lmmse_seq_estimate_host
from helpers import TOL_HIP_MSE
from test_chansim_gpu import _bits, _no_sync, _poison, _same_bits
from test_lmmse_gpu import U, _conds, _dev, _gamma

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _windows(tb: LmmseTables, pilots: np.ndarray):
    """Per frame of whole sequences: (w, the window's pilots [Ps, w Pt] or None)."""
    K, G, (Ps, Pt) = tb.cfg.slots, tb.cfg.group, tb.cfg.pilot
    for n in range(len(pilots)):
        w = int(tb.slot_window(n // G % K))
        src = [n - (tb.horizon + w - 1 - i) * G for i in range(w)]
        yield w, (np.concatenate([pilots[s] for s in src], axis=1) if w else None)


def seq_bound(tb: LmmseTables, pilots: np.ndarray, idx) -> np.ndarray:
    """Bound on |device estimate - definition| per element, [n, S, T]; module docstring."""
    Ps, Pt = tb.cfg.pilot
    r2 = np.sqrt(2.0)
    cc = (1 + U) * (1 + r2 * _gamma(2 * Ps)) - 1          # complex x complex stage of Ps terms, rounded table
    ex = (1 + U) ** 3 - 1
    r_d = (1 + ex / (1 - ex)) * (1 + 5 * U) - 1
    out = np.zeros((len(pilots), *tb.cfg.ofdm))
    for n, ((w, p), a, d, e) in enumerate(zip(_windows(tb, pilots), *idx)):
        if w == 0:
            continue
        cr = (1 + U) * (1 + _gamma(w * Pt)) - 1           # complex x real stage of w Pt terms, rounded table
        _, u_t, t_p = tb.time(e, w)
        ufh, ut, tp, fp, gain = np.abs(tb.u_f[d].conj().T), np.abs(u_t), np.abs(t_p), np.abs(tb.f[d]), tb.gain(a, d, e, w)
        a1 = ufh @ np.abs(p)
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


# name: (config, W, h, sequences)
CASES = {
    "default_every_w": (ChannelSimConfig(slots=4), 4, 0, 3),                                             # every w from 1 to 4 occurs
    "default_predict": (ChannelSimConfig(slots=4), 2, 1, 3),                                             # a zero slot, then w = 1, then w = 2
    "odd_30x7_group_gap": (ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3), slots=3, antennas=(1, 2), slot_symbols=9), 3, 0, 3),
    "three_tiles_24x37": (ChannelSimConfig(ofdm=(24, 37), pilot=(4, 5), slots=6), 6, 0, 2),              # w Pt = 30
    "lds_bound_128x40": (ChannelSimConfig(ofdm=(128, 40), pilot=(64, 16), slots=2), 2, 0, 2),            # w Pt = 32: LDS at its bound
    "degenerate_1x1_group_16": (ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1), slots=3, antennas=(4, 4)), 3, 2, 2),   # w stays 1, two zero slots
    # either side of the threshold between the kernel's two instantiations (W Pt <= 16: 24 KB of LDS; above: 40 KB)
    "default_w8_narrow_tiles": (ChannelSimConfig(slots=9), 8, 0, 1),                                     # W Pt = 16
    "default_w9_wide_tiles": (ChannelSimConfig(slots=9), 9, 0, 1),                                       # W Pt = 18
}
_cache = {}


def _case(name):
    """(cfg, tables, plan, pilots complex64 [b,Ps,Pt], meta float32 [b,3], definition complex128 [b,S,T]), made once per case."""
    if name not in _cache:
        cfg, W, h, seqs = CASES[name]
        tb = LmmseTables(cfg, W, h)
        _, pilots, meta = simulate_frames_host(cfg, 11, np.arange(seqs * cfg.sequence()))
        pilots = pilots.astype(np.complex64)
        want = lmmse_seq_estimate_host(tb, pilots, meta)
        for a in (pilots, meta, want):
            a.setflags(write=False)
        _cache[name] = (cfg, tb, LmmseSeqPlan(tb, DEV), pilots, meta, want)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_float64_definition(name):
    cfg, tb, plan, pilots, meta, want = _case(name)
    b = len(pilots)
    assert plan.image.numel() == _lib.load().aft_lmmse_seq_table_floats(ctypes.byref(plan.plan), tb.window)
    bound = seq_bound(tb, pilots, tb.indices(meta))
    ws = tb.slot_window(np.arange(b) // cfg.group % cfg.slots)
    assert sorted(set(ws.tolist())) == {"default_every_w": [1, 2, 3, 4], "default_predict": [0, 1, 2], "odd_30x7_group_gap": [1, 2, 3],
                                        "three_tiles_24x37": [1, 2, 3, 4, 5, 6], "lds_bound_128x40": [1, 2],
                                        "degenerate_1x1_group_16": [0, 1], "default_w8_narrow_tiles": list(range(1, 9)),
                                        "default_w9_wide_tiles": list(range(1, 10))}[name]
    _poison([((b, *cfg.ofdm), torch.complex64)])                  # an element the kernel leaves unwritten would come back NaN
    est = plan(_dev(pilots), *_conds(meta))
    assert est.shape == want.shape and est.dtype == torch.complex64 and est.is_cuda
    got = est.cpu().numpy().astype(np.complex128)
    assert np.isfinite(got).all()
    err, scale = np.abs(got - want), float(np.abs(want).max())
    live = ws > 0
    print(f"{name}: max|est - def| {err.max():.3e} = {err.max() / scale:.3e} |h|max   largest err / bound "
          f"{float((err[live] / bound[live]).max()):.3f}   (bound up to {bound.max():.3e} = {bound.max() / scale:.3e} |h|max)")
    assert (err <= bound).all()
    assert not _bits(est[torch.from_numpy(~live).to(DEV)]).any()          # no window: +0.0 in both components


def test_window_1_horizon_0_is_the_single_slot_kernel():
    cfg = ChannelSimConfig(slots=4)
    _, pilots, meta = simulate_frames_host(cfg, 12, np.arange(20))
    pil, conds = _dev(pilots.astype(np.complex64)), _conds(meta)
    tb = LmmseTables(cfg, 1, 0)
    seq = LmmseSeqPlan(tb, DEV)
    single = LmmsePlan(tb, DEV)
    assert torch.equal(seq.image, single.image)
    _same_bits([seq(pil, *conds)], [single(pil, *conds)])
    odd = ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3), slots=3, antennas=(1, 2), slot_symbols=9)
    _, pilots, meta = simulate_frames_host(odd, 12, np.arange(12))
    pil, conds = _dev(pilots.astype(np.complex64)), _conds(meta)
    _same_bits([LmmseSeqPlan(LmmseTables(odd), DEV)(pil, *conds)], [LmmsePlan(odd, DEV)(pil, *conds)])


def test_the_two_instantiations_give_the_same_bits():
    """W Pt <= 16 runs on the narrow LDS tiles, anything above on the wide ones: slots 0 .. 7 of a 9-slot sequence have the same
    windows and the same tables under W = 8 and W = 9, so their bits must not tell the two kernels apart."""
    _, tb8, narrow, pilots, meta, _ = _case("default_w8_narrow_tiles")
    _, tb9, wide, pilots9, meta9, _ = _case("default_w9_wide_tiles")
    assert np.array_equal(pilots, pilots9) and np.array_equal(meta, meta9)
    assert all(np.array_equal(x, y) for w in range(1, 9) for x, y in zip(tb8.time(0, w), tb9.time(0, w)))
    _same_bits([narrow(_dev(pilots), *_conds(meta))[:8]], [wide(_dev(pilots), *_conds(meta))[:8]])


def test_a_slot_depends_on_its_window_only():
    """Slot k >= W - 1 of a K-slot sequence equals the last slot of the W-slot sequence cut from its pilots; a sequence alone equals
    itself at positions 1 and 4 of a 5-sequence batch."""
    for name in ("default_every_w", "odd_30x7_group_gap"):
        cfg, tb, plan, pilots, meta, _ = _case(name)
        K, G, W, unit = cfg.slots, cfg.group, tb.window, cfg.sequence()
        full = plan(_dev(pilots), *_conds(meta))
        W = 2 if name == "default_every_w" else W
        short_cfg = dataclasses.replace(cfg, slots=W)
        long_tb = LmmseTables(cfg, W, 0)
        long_plan = LmmseSeqPlan(long_tb, DEV)
        full_w = long_plan(_dev(pilots), *_conds(meta))
        short = LmmseSeqPlan(LmmseTables(short_cfg, W, 0), DEV)
        for k in range(W - 1, K):
            lo, hi = (k - W + 1) * G, (k + 1) * G                 # the window's frames of sequence 0
            cut = short(_dev(pilots[lo:hi]), *_conds(meta[lo:hi]))
            _same_bits([cut[-G:]], [full_w[k * G:(k + 1) * G]])
        alone = plan(_dev(pilots[:unit]), *_conds(meta[:unit]))
        _same_bits([alone], [full[:unit]])
        _, many_p, many_m = simulate_frames_host(cfg, 13, np.arange(5 * unit))
        many_p = many_p.astype(np.complex64)
        for pos in (1, 4):
            many_p[pos * unit:(pos + 1) * unit], many_m[pos * unit:(pos + 1) * unit] = pilots[:unit], meta[:unit]
        batch = plan(_dev(many_p), *_conds(many_m))
        _same_bits([batch[unit:2 * unit], batch[4 * unit:]], [alone, alone])


def test_pinned_inputs_null_conditions_and_the_8_byte_store_form():
    cfg, tb, plan, pilots, meta, _ = _case("default_every_w")
    b = len(pilots)
    pil, conds = _dev(pilots), _conds(meta)
    want = plan(pil, *conds)
    _same_bits([plan(torch.from_numpy(np.array(pilots)).pin_memory(), *_conds(meta, "pinned"))], [want])
    # assume= with NULL condition pointers against explicit conditions at those values
    assume = dict(snr_db=10, delay_spread_ns=350, doppler_hz=1400)
    pinned = LmmseSeqPlan(tb, DEV, assume=assume)
    flat = np.tile(np.array([[10, 350, 1400]], dtype=np.float32), (b, 1))
    _same_bits([pinned(pil)], [plan(pil, *_conds(flat))])
    _same_bits([pinned(pil, *conds)], [plan(pil, *_conds(flat))])                      # ... and given arrays are not read
    with pytest.raises(ValueError, match="ds is required"):
        plan(pil, conds[0], None, conds[2])
    with pytest.raises(ValueError, match="HIP device"):
        LmmseSeqPlan(tb, "cpu")
    with pytest.raises(ValueError, match="table image"):
        LmmseSeqPlan(tb, DEV, image=plan.image[:-1])
    # a base 8 bytes off 16 goes through the entry point directly (the caching allocator only hands out 512-byte aligned blocks)
    out = torch.empty((b * 120 * 14 + 1,), dtype=torch.complex64, device=DEV)
    torch.view_as_real(out).fill_(float("nan"))
    assert (out.data_ptr() + 8) % 16 == 8
    _lib.check(_lib.load().aft_lmmse_seq_f32(ctypes.byref(plan.plan), 1, 4, 4, 0, plan.image.data_ptr(), pil.data_ptr(),
                                             *(c.data_ptr() for c in conds), out.data_ptr() + 8, b, _lib.current_stream_ptr(out.device)))
    _same_bits([out[1:].view(b, 120, 14)], [want])
    assert torch.isnan(torch.view_as_real(out[:1])).all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_lmmse_seq_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_lmmse_seq_f32")
    for name in CASES:
        cfg, tb, plan, pilots, meta, _ = _case(name)
        _same_bits([plan(_dev(pilots), *_conds(meta), lib=lib)], [plan(_dev(pilots), *_conds(meta))])


def test_no_read_of_a_slot_outside_the_window_and_exact_zeros():
    cfg, tb, plan, pilots, meta, _ = _case("default_every_w")
    want = plan(_dev(pilots), *_conds(meta))
    for k in range(3):                                            # the pilots of every slot after k are NaN: slots 0 .. k do not see them
        later = np.array(pilots)
        later.reshape(3, 4, 12, 2)[:, k + 1:] = np.nan
        got = plan(_dev(later), *_conds(meta))
        keep = torch.from_numpy(np.arange(12) % 4 <= k).to(DEV)
        assert torch.isfinite(torch.view_as_real(got[keep])).all()
        _same_bits([got[keep]], [want[keep]])
    cfg, tb, plan, pilots, meta, _ = _case("default_predict")    # h = 1: slot k looks at slots up to k - 1; slot 0 at nothing
    want = plan(_dev(pilots), *_conds(meta))
    for k in range(4):
        later = np.array(pilots)
        later.reshape(3, 4, 12, 2)[:, k:] = np.nan
        nan_meta = np.array(meta)
        nan_meta[0::4] = np.nan                                   # ... and slot 0 does not read its conditions either
        _poison([((12, 120, 14), torch.complex64)])
        got = plan(_dev(later), *_conds(nan_meta))
        keep = torch.from_numpy((np.arange(12) % 4 <= k) & (np.arange(12) % 4 > 0)).to(DEV)
        _same_bits([got[keep]], [want[keep]])
        assert not _bits(got[0::4]).any()                         # +0.0 in both components


def test_module_runs_from_the_loaders_without_a_synchronisation():
    cfg = ChannelSimConfig(slots=4, antennas=(1, 2))
    model = LmmseEstimator(cfg, window=4).to(DEV).eval()
    assert model.table_image.is_cuda and list(model.parameters()) == [] and list(model.steady_slots()) == [3]
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
        assert est.is_cuda and est.shape == ideal.shape and est.dtype == torch.complex64
        cond = np.concatenate([m.cpu().numpy() for m in meta[1:4]], axis=1)
        p = pil.cpu().numpy()
        want = lmmse_seq_estimate_host(tb, p, cond)
        assert (np.abs(est.cpu().numpy() - want) <= seq_bound(tb, p, tb.indices(cond))).all()
    # CPU-tensor batches go through the pinned ring: the same bits as device-resident inputs, for more batches than the ring has slots
    pack = make_pack(cfg, 80, seed=6)
    host_batches = list(ingest.ResidentLoader(pack, cfg.pilot, 8, device="cpu", shuffle=False))
    assert len(host_batches) == 10 and not host_batches[0][0].is_cuda
    resident = [model(p.to(DEV), tuple(m.to(DEV) if torch.is_tensor(m) else m for m in meta)) for p, _, meta in host_batches]
    torch.cuda.synchronize()
    with _no_sync():
        ringed = [model(p, meta) for p, _, meta in host_batches]
    _same_bits(ringed, resident)
    with pytest.raises(ValueError, match="need whole sequences in order"):
        model(host_batches[0][0][:6], None)


def test_evaluation_sweep_over_simulated_packs():
    from adafortitran_amd.evaluation import get_test_stats
    cfg = ChannelSimConfig(slots=4)
    packs = {snr: make_pack(cfg, 256, seed=20 + snr, snr_db=snr) for snr in (0, 10, 20)}
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    stats = {}
    for W in (1, 4):
        model = LmmseEstimator(cfg, window=W).to(DEV)
        loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, cfg.pilot, 128, device=DEV, shuffle=False)) for snr, pack in packs.items()]
        stats[W] = get_test_stats(model, loaders)
        assert list(stats[W]) == [0, 10, 20]
    tb = LmmseTables(cfg, 4, 0)
    for snr, pack in packs.items():
        pil = pack["h_ls_sparse"][:, sc[:, None], sym[None, :]]
        want = lmmse_seq_estimate_host(tb, pil, pack["meta"][:, 1:4])
        mse = float((np.abs(want - pack["h_ideal"]) ** 2).mean())
        got, one = 10.0 ** (stats[4][snr] / 10.0), 10.0 ** (stats[1][snr] / 10.0)
        print(f"SNR {snr}: W = 4 on the device {got:.6e}  definition {mse:.6e}  |d|/MSE {abs(got - mse) / mse:.3e}   W = 1 {one:.6e}")
        assert abs(got - mse) <= TOL_HIP_MSE * mse
        assert got < one


def test_every_refusal_of_the_entry_point_launches_nothing():
    cfg, tb, plan, pilots, meta, _ = _case("default_every_w")
    lib, b = _lib.load(), len(pilots)
    est = torch.empty((b, 120, 14), dtype=torch.complex64, device=DEV)
    torch.view_as_real(est).fill_(float("nan"))
    pil, conds = _dev(pilots), _conds(meta)
    good = dict(group=1, slots=4, window=4, horizon=0, tables=plan.image.data_ptr(), pilots=pil.data_ptr(), snr=conds[0].data_ptr(),
                ds=conds[1].data_ptr(), dop=conds[2].data_ptr(), est=est.data_ptr(), batch=b)

    def call(p=None, **kw):
        a = dict(good, **kw)
        return lib.aft_lmmse_seq_f32(ctypes.byref(p if p is not None else tb.to_struct()), a["group"], a["slots"], a["window"], a["horizon"],
                                     a["tables"], a["pilots"], a["snr"], a["ds"], a["dop"], a["est"], a["batch"], None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_lmmse_seq_f32(None, 1, 4, 4, 0, good["tables"], good["pilots"], good["snr"], good["ds"], good["dop"], good["est"], b, None)
    assert rc == E and "NULL" in lib.aft_last_error().decode()
    for k in ("tables", "pilots", "est"):
        refused(E, "NULL pointer", **{k: None})
        refused(E, "8-byte", **{k: good[k] + 4})
    for k in ("snr", "ds", "dop"):
        refused(E, "NULL condition", **{k: None})
        refused(E, "4-byte", **{k: good[k] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for batch in (b - 1, 6):
        refused(E, "is not a multiple of slots * group = 4 * 1", batch=batch)
    refused(E, "is not a multiple of slots * group = 4 * 2", group=2, batch=4)
    for field, value, word in (("num_scs", 0, "num_scs = 0"), ("pilot_symbols", 17, "pilot_symbols = 17 is outside 1..16"),
                               ("n_dop", 17, "n_dop = 17"), ("fixed_snr", 7, "fixed_snr = 7 is outside -1..6"),
                               ("num_symbols", 1, "larger than the ofdm grid")):
        p = tb.to_struct()
        setattr(p, field, value)
        refused(SH, word, p=p)
        assert lib.aft_lmmse_seq_table_floats(ctypes.byref(p), 4) == 0
    for kw, word in ((dict(group=0), "group = 0 is outside 1..16"), (dict(group=17), "group = 17 is outside 1..16"),
                     (dict(slots=0), "slots = 0 is outside 1..4096"), (dict(slots=4097, window=4), "slots = 4097 is outside 1..4096"),
                     (dict(window=0), "window = 0 is outside 1..4"), (dict(window=5), "window = 5 is outside 1..4"),
                     (dict(slots=32, window=17), "window * pilot_symbols = 34 is outside 1..32"),
                     (dict(horizon=-1), "horizon = -1 is outside 0..3"), (dict(horizon=4), "horizon = 4 is outside 0..3")):
        refused(SH, word, **kw)
    for window in (0, -1, 17, 5000):
        assert lib.aft_lmmse_seq_table_floats(ctypes.byref(tb.to_struct()), window) == 0
    assert lib.aft_lmmse_seq_table_floats(None, 4) == 0
    torch.cuda.synchronize()
    assert torch.isnan(torch.view_as_real(est)).all()                                # nothing was launched
    blocks = sum(2 * w * (2 * w + 14 + 1) for w in range(1, 5))
    assert lib.aft_lmmse_seq_table_floats(ctypes.byref(tb.to_struct()), 4) == plan.image.numel() == 7 * (2 * 144 + 2 * 12 * 120 + 12) + 7 * blocks
    assert lib.aft_lmmse_seq_table_floats(ctypes.byref(tb.to_struct()), 1) == lib.aft_lmmse_table_floats(ctypes.byref(tb.to_struct()))
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(est)).all()                             # ... and the good call writes it all
