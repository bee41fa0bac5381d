"""``aft_link_observe_f32``, ``hip_ops.LinkObservePlan``, ``linksim.DataAidedRefiner`` and the ``refine=`` keyword of the sweeps on the
HIP device: the kernel's decisions against the float64 definition except where flagged, z against the definition ON THE DEVICE'S OWN
DECISIONS within the bound derived below, the pilots bit for bit, independence of the batch, of the position and of the run, no
unwritten element, bases off 16 bytes, the checked build, the refusals, the refiner against the CPU refiner without a synchronisation,
and the refined sweep against the unrefined one.

Shapes: tests/test_linkdd.py's ``dd_inputs`` (seed 3; every frame at the SNR it was drawn with, so the weights are mixed) with R = 1, 2
and 4 where the frames allow it (3 x 5 has four frames, 300 x 4 two).

The decisions.  c and p are ``aft_link_mrc_f32``'s chain on the same operands, so a decision can differ from the definition's only where
tests/test_linkmrc_gpu.py's ``derived_tau(R)`` flags the (element, axis) pair; the flagged share stays within ``SHARE_CAP`` and the
symbol-error count is within the flagged elements of the definition's.

The bound on z (``derived_z_bound``), per data element, u = 2^-24, no fast-math:
* y: tests/test_linksim_gpu.py's chain gives |y_dev - y| <= e_y (|H||x| + |noise|) with e_y as in its ``derived_tau`` (the rounding of
  d, the two products, the Box-Muller radius and angle, the two fused multiply-adds);
* x^ = float32(d) k: one rounding of d, one of the product: e_x = (1 + u)^2 - 1 per component;
* a component of the numerator, fma(yr, ar, yi ai): the inputs' errors e_y r_y |x^| (1 + e_x) + |y| e_x |x^|, plus two roundings of
  a sum of products bounded by |y_dev||x^_dev|: eN in all (|a_r b_r| + |a_i b_i| <= |a||b|);
* |x^|^2 = fma(ar, ar, ai ai): non-negative terms, two roundings on squared inputs: e_d = (1 + e_x)^2 (1 + u)^2 - 1;
* one correctly rounded division: (1 + u).
A component errs by at most ((N + eN) (1 + u) / (1 - e_d) - N) / |x^|^2 with N = |y||x^|; the modulus by sqrt(2) times that."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, ls_interpolate, make_pack
from adafortitran_amd.evaluation import get_link_stats
from adafortitran_amd.hip_ops import LinkMrcPlan, LinkObservePlan
from adafortitran_amd.linksim import (DEFAULT_FACTORS, PILOT_DECISION, DataAidedRefiner, LinkConfig, _noise, _sent, branch_weights,
                                      data_noise_scale, link_observe_host, noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator, LmmseTables, lmmse_estimate_host
from test_chansim_gpu import _no_sync, _same_bits
from test_linkdd import DD_GRIDS, dd_inputs
from test_linkmrc_gpu import derived_tau
from test_linksim import SHARE_CAP, flagged_share
from test_linksim_gpu import U, _dev
from test_lmmse_grid_gpu import derived_grid_bound, nan_complex

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7777
CASES = (("default_120x14", (1, 2, 4)), ("odd_30x7", (1, 2, 4)), ("odd_last_alone_3x5", (1, 2, 4)), ("tall_300x4", (1, 2)))
MS = (2, 4, 6, 8)                                                               # 8: the L = 16 instantiation, where 255 is also (15, 15)


def _e_y() -> float:
    """The relative error of the device's received sample, in units of |H||x| + |noise|: the first five lines of ``derived_tau``."""
    e_x = (1 + U) ** 2 - 1
    e_h = (1 + e_x) * (1 + U) ** 2 - 1
    e_r = (1 + 3 * U) * (1 + 6 * U) * (1 + U) - 1
    e_n = e_r + 8 * U * (1 + e_r)
    return float(max(e_h, e_n) + U * (1 + e_n))


def derived_z_bound(cfg, keys, ideal, sigma, decisions, R, sent=False) -> np.ndarray:
    """Bound on |z_dev - z_def| per element, [n, S, T] (0 at the pilots: they are copied); module docstring."""
    e_y, e_x = _e_y(), (1 + U) ** 2 - 1
    e_d = (1 + e_x) ** 2 * (1 + U) ** 2 - 1
    L, d, mask = cfg.levels, cfg.d, cfg.data_mask
    gi, gq, x = _sent(cfg, keys[::R])
    ki, kq = (decisions & 15).astype(np.int64), (decisions >> 4).astype(np.int64)
    xh = np.where(mask[None], x if sent else d * ((2 * ki - (L - 1)) + 1j * (2 * kq - (L - 1))), 1.0)
    out = np.zeros(ideal.shape)
    for r in range(R):
        noise = _noise(cfg, keys[r::R], sigma[r::R].astype(np.float64))
        H = ideal[r::R].astype(np.complex128)
        reach, y, ax = np.abs(H) * np.abs(x) + np.abs(noise), np.abs(H * x + noise), np.abs(xh)
        N = y * ax
        eN = e_y * reach * ax * (1 + e_x) + y * e_x * ax + 2 * U * (y + e_y * reach) * (1 + e_x) * ax
        out[r::R] = np.sqrt(2.0) * ((N + eN) * (1 + U) / (1 - e_d) - N) / ax ** 2 * mask[None]
    return out


_plans, _ops = {}, {}


def _same(a, b):
    """``_same_bits`` for tuples that hold the uint8 decision map (widened first: a row of bytes need not be whole int32 words)."""
    wide = lambda ts: [t.to(torch.int32) if t.dtype == torch.uint8 else t for t in ts]  # noqa: E731
    _same_bits(wide(a), wide(b))


def _plan(name, m, R, source="decided"):
    if (name, m, R, source) not in _plans:
        _plans[name, m, R, source] = LinkObservePlan(LinkConfig(dd_inputs(name)[0], m), DEV, R, source)
    return _plans[name, m, R, source]


def _operands(name, R):
    """The host operands (keys, sigma, rho, scale, ideal, est, pilots) and the device's (ideal, est, keys, sigma, rho, pilots)."""
    if (name, R) not in _ops:
        sim, keys, sigma, snr, ideal, pilots, meta, est = dd_inputs(name)
        rho, scale = branch_weights(snr, 0.0, R)
        _ops[name, R] = ((keys, sigma, rho, scale, ideal, est, pilots), tuple(_dev(a) for a in (ideal, est, keys, sigma, rho, pilots)))
    return _ops[name, R]


def _run(name, m, R, source="decided", lib=None):
    return _plan(name, m, R, source)(*_operands(name, R)[1], lib=lib)


@pytest.mark.parametrize("m", MS)
def test_kernel_against_the_float64_definition(m):
    groups = flagged_groups = differing = 0
    worst = 0.0
    for name, branches in CASES:
        sim = dd_inputs(name)[0]
        cfg = LinkConfig(sim, m)
        sc, sym = np.asarray(sim.pilot_scs), np.asarray(sim.pilot_symbols)
        for R in branches:
            (keys, sigma, rho, scale, ideal, est, pilots), _ = _operands(name, R)
            n, G = len(keys), len(keys) // R
            _, want_dec, want_err, flags = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots, R, tau=derived_tau(R))
            assert flagged_share(cfg, flags) <= SHARE_CAP
            z, dec, err = _run(name, m, R)
            assert z.shape == (n, *sim.ofdm) and z.dtype == torch.complex64 and dec.shape == (G, *sim.ofdm) and dec.dtype == torch.uint8
            assert err.shape == (G,) and err.dtype == torch.int32
            got_z, got_dec, got_err = z.cpu().numpy(), dec.cpu().numpy(), err.cpu().numpy().astype(np.int64)
            elems = flags.any(axis=3)
            assert (got_dec[~elems] == want_dec[~elems]).all(), (name, R, int((got_dec != want_dec).sum()), int(elems.sum()))
            assert (got_dec[:, ~cfg.data_mask] == PILOT_DECISION).all()
            assert (got_err >= 0).all() and (np.abs(got_err - want_err) <= elems.sum(axis=(1, 2))).all(), (name, R, got_err, want_err)
            assert (got_z[:, sc[:, None], sym[None, :]].view(np.int64) == pilots.view(np.int64)).all()      # the pilots, bit for bit
            for source in ("decided", "sent"):
                zs = got_z if source == "decided" else _run(name, m, R, "sent")[0].cpu().numpy()
                want_z = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots, R, source=source, decisions=got_dec)[0]
                bound = derived_z_bound(cfg, keys, ideal, sigma, got_dec, R, sent=source == "sent")
                e = np.abs(zs.astype(np.complex128) - want_z)
                assert np.isfinite(zs).all() and (e <= bound).all(), (name, R, source, float((e / np.where(bound > 0, bound, 1)).max()))
                worst = max(worst, float((e[bound > 0] / bound[bound > 0]).max(initial=0.0)))
            groups += G
            flagged_groups += int(elems.any(axis=(1, 2)).sum())
            differing += int((got_dec != want_dec).any(axis=(1, 2)).sum())
    print(f"m = {m}: {flagged_groups} of {groups} groups had a flagged decision at tau(R); {differing} differ from the definition; "
          f"largest |z_dev - z_def| / bound = {worst:.3f}")


@pytest.mark.parametrize("m", MS)
def test_the_decisions_are_the_diversity_kernels(m):
    """The count is ``aft_link_mrc_f32``'s symbol-error count on the same operands, exactly: the same chain, the same decision."""
    f = _dev(np.asarray(DEFAULT_FACTORS[:1], dtype=np.float32))
    for name, branches in CASES:
        for R in branches:
            (_, _, _, scale, *_), (h, e, k, s, rho, p) = _operands(name, R)
            counts, _, _ = LinkMrcPlan(LinkConfig(dd_inputs(name)[0], m), DEV, R)(h, e, k, s, rho, _dev(scale), f)
            assert torch.equal(_run(name, m, R)[2], counts[:, 1])


def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run():
    m = 4
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, snr, ideal, pilots, meta, est = dd_inputs(name)
        for R in (1, 2, 4):
            p = _plan(name, m, R)
            idx = (np.arange(37 * R) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-R:] = np.arange(R, 2 * R)                                       # ... the last one group 1 of ``_operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est[i]), _dev(keys[i]), _dev(sigma[i]), _dev(branch_weights(snr[i], 0.0, R)[0]),  # noqa: E731
                             _dev(pilots[i]))
            batch, alone = p(*ops(idx)), p(*ops(np.arange(R, 2 * R)))
            _same([batch[0][36 * R:], batch[1][36:], batch[2][36:]], alone)
            want = _run(name, m, R)
            _same([want[0][R:2 * R], want[1][1:2], want[2][1:2]], alone)
            _same(p(*ops(idx)), batch)                                      # a second run of the same batch


def _entry(plan, ptrs, z, dec, err, batch, lib=None, struct=None, source=None, branches=None):
    h, e, k, s, rho, p = ptrs
    lib = lib or _lib.load()
    return lib.aft_link_observe_f32(ctypes.byref(plan.link if struct is None else struct), h, e, k, s, rho, p,
                                    plan.source if source is None else source, plan.branches if branches is None else branches, z, dec, err,
                                    batch, _lib.current_stream_ptr(torch.device(DEV, torch.cuda.current_device())))


def test_poisoned_outputs_and_bases_off_16_bytes():
    """Every element of the three outputs is written and nothing beside them; with ideal, est and z 8 bytes off a 16-byte boundary (the
    8-byte loads and stores) the same bits; the odd grid's last element, alone in its pair, is written for every branch."""
    m = 4
    for name, R in (("default_120x14", 2), ("odd_30x7", 4), ("odd_last_alone_3x5", 2), ("tall_300x4", 1)):
        plan, ops = _plan(name, m, R), _operands(name, R)[1]
        want = _run(name, m, R)
        n, G, frame = want[0].shape[0], want[1].shape[0], want[1][0].numel()
        h, e = ops[0], ops[1]
        fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
        fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
        ptrs = [t.data_ptr() for t in ops]
        for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 1), (None, fe.data_ptr() + 8, 0), (fh.data_ptr() + 8, None, 1)):
            z = nan_complex((n * frame + 2,))
            dec = torch.full((G * frame + 16,), 99, dtype=torch.uint8, device=DEV)
            err = torch.full((G + 1,), POISON, dtype=torch.int32, device=DEV)
            p = [hp or ptrs[0], ep or ptrs[1], *ptrs[2:]]
            _lib.check(_entry(plan, p, z.data_ptr() + 8 * off, dec.data_ptr(), err.data_ptr(), n))
            _same([z[off:off + n * frame], dec[:G * frame].to(torch.int32), err[:G]], [want[0].reshape(-1), want[1].reshape(-1).to(torch.int32), want[2]])
            assert torch.view_as_real(z[:off]).isnan().all() and torch.view_as_real(z[off + n * frame:]).isnan().all()
            assert (dec[G * frame:] == 99).all() and (err[G:] == POISON).all()
    z, dec, _ = _run("odd_last_alone_3x5", m, 2)
    assert torch.view_as_real(z).isfinite().all() and (dec[:, 2, 4] != PILOT_DECISION).all() and (dec[:, 1, 2] == PILOT_DECISION).all()


def test_checked_build_gives_the_same():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_observe_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION
    for name, branches in CASES:
        for m in MS:
            for R in branches:
                _same(_run(name, m, R, lib=lib), _run(name, m, R))
    _same(_run("odd_30x7", 4, 2, "sent", lib=lib), _run("odd_30x7", 4, 2, "sent"))


def test_what_the_plan_refuses():
    name, m, R = "odd_30x7", 4, 4
    cfg = LinkConfig(dd_inputs(name)[0], m)
    h, e, k, s, rho, p = _operands(name, R)[1]
    plan = _plan(name, m, R)
    for args, word in (((h[:6], e[:6], k[:6], s[:6], rho[:6], p[:6]), "6 frames is not a multiple of branches = 4"),
                       ((h, e, k, s, rho[:7], p), "rho must hold"), ((h, e, k, s, rho.double(), p), "rho must be torch.float32"),
                       ((h, e, k, s, rho, p[:, :4]), "pilots must be complex64"), ((h, e, k, s, rho, p.cpu()), "pilots must be complex64")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkObservePlan(cfg, DEV, bad)
    with pytest.raises(ValueError, match='"decided"'):
        LinkObservePlan(cfg, DEV, 1, "soft")
    with pytest.raises(ValueError, match="LinkObservePlan runs on a HIP device"):
        LinkObservePlan(cfg, "cpu", 1)


def test_every_refusal_of_the_entry_point_launches_nothing():
    name, m, R = "default_120x14", 4, 2
    cfg = LinkConfig(dd_inputs(name)[0], m)
    plan, ops = _plan(name, m, R), _operands(name, R)[1]
    lib, n = _lib.load(), ops[0].shape[0]
    z = nan_complex((n, *cfg.sim.ofdm))
    dec = torch.full((n // R, *cfg.sim.ofdm), 99, dtype=torch.uint8, device=DEV)
    err = torch.full((n // R,), POISON, dtype=torch.int32, device=DEV)
    good = [t.data_ptr() for t in ops]
    names = ("ideal", "est", "keys", "sigma", "rho", "pilots")
    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE

    def refused(code, word, rc):
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    def call(swap=None, z_=None, dec_=None, err_=None, batch=n, **kw):
        ptrs = list(good)
        for key, value in (swap or {}).items():
            ptrs[names.index(key)] = value
        return _entry(plan, ptrs, z.data_ptr() if z_ is None else z_, dec.data_ptr() if dec_ is None else dec_,
                      err.data_ptr() if err_ is None else err_, batch, **kw)

    refused(E, "NULL pointer", lib.aft_link_observe_f32(None, *good, 0, R, z.data_ptr(), dec.data_ptr(), err.data_ptr(), n, None))
    for x in names:
        refused(E, "NULL pointer", _entry(plan, [None if y == x else g for y, g in zip(names, good)], z.data_ptr(), dec.data_ptr(), err.data_ptr(), n))
    for kw in (dict(z_=0), dict(dec_=0), dict(err_=0)):
        refused(E, "NULL pointer", _entry(plan, good, kw.get("z_", z.data_ptr()) or None, kw.get("dec_", dec.data_ptr()) or None,
                                          kw.get("err_", err.data_ptr()) or None, n))
    for x in ("ideal", "est", "keys", "pilots"):
        refused(E, "8-byte", call({x: good[names.index(x)] + 4}))
    refused(E, "8-byte", call(z_=z.data_ptr() + 4))
    for x in ("sigma", "rho"):
        refused(E, "4-byte", call({x: good[names.index(x)] + 2}))
    refused(E, "4-byte", call(err_=err.data_ptr() + 2))
    for batch in (0, -3):
        refused(E, "batch must be at least 1", call(batch=batch))
    for bad in (0, 9, -2):
        refused(SH, f"branches = {bad} is outside 1..8", call(branches=bad))
    refused(E, "batch = 16 is not a multiple of branches = 3", call(branches=3))
    for bad in (2, -1):
        refused(E, f"source = {bad} is neither", call(source=bad))
    for fields, word in ((dict(num_scs=0), "num_scs = 0"), (dict(pilot_scs=65), "pilot_scs = 65 is outside 1..64"),
                         (dict(num_symbols=1), "larger than the ofdm grid"), (dict(bits_per_symbol=3), "bits_per_symbol = 3")):
        p = cfg.to_struct()
        for key, value in fields.items():
            setattr(p, key, value)
        refused(SH, word, call(struct=p))
    torch.cuda.synchronize()
    assert torch.view_as_real(z).isnan().all() and (dec == 99).all() and (err == POISON).all()      # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    _same([z, dec.to(torch.int32), err], [t.to(torch.int32) if t.dtype == torch.uint8 else t for t in _run(name, m, R)])
    # a grid whose every element is a pilot is legal: z is the pilots, no decision, no error
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    assert call(struct=one, batch=4) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert torch.equal(z.reshape(-1)[:4], ops[5].reshape(-1)[:4]) and dec.reshape(-1)[:2].tolist() == [PILOT_DECISION] * 2
    assert err[:2].tolist() == [0, 0]


def test_the_refiner_on_the_device_against_the_cpu_refiner_without_a_synchronisation():
    """One 32-frame pack at 20 dB, 16-QAM, the SAME complex64 LMMSE estimate into both refiners, one pass.  The decisions differ at
    flagged elements only, so the counts agree within the flagged elements; the estimates differ by the z bound pushed through the
    smoother (a contraction in l2: its eigenvalues g_kl are below 1), the smoother's own bound, and one complex64 rounding of the twin's
    result -- plus, per flagged element, a z that may have moved by 2 |y| / |x|min.  |sqrt(NMSE_dev) - sqrt(NMSE_cpu)| is at most the
    rms of that difference over rms(h)."""
    sim, seed, m = ChannelSimConfig(), 9, 4
    cfg, tb = LinkConfig(sim, m), LmmseTables(sim)
    pack = make_pack(sim, 32, seed=31, snr_db=20)
    sc, sym = np.asarray(sim.pilot_scs), np.asarray(sim.pilot_symbols)
    ideal, meta = pack["h_ideal"].astype(np.complex64), pack["meta"][:, 1:4]
    pilots = np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]]).astype(np.complex64)
    est = lmmse_estimate_host(tb, pilots, meta).astype(np.complex64)
    ids = torch.arange(32)
    metas = (ids.float(), *(torch.from_numpy(meta[:, k].copy()) for k in range(3)))
    host, dev = DataAidedRefiner(cfg, "cpu", seed), DataAidedRefiner(cfg, DEV, seed)
    want = host.refine(torch.from_numpy(est), torch.from_numpy(pilots), torch.from_numpy(ideal), metas).numpy()
    e_d, p_d, h_d = _dev(est), _dev(pilots), _dev(ideal)
    metas_d = tuple(t.to(DEV) for t in metas)
    dev.refine(e_d, p_d, h_d, metas_d)                                            # warm: the plans, the allocator
    dev = DataAidedRefiner(cfg, DEV, seed)
    two = DataAidedRefiner(cfg, DEV, seed, iterations=2)
    with _no_sync():
        got = dev.refine(e_d, p_d, h_d, metas_d)
        got2 = two.refine(e_d, p_d, h_d, metas_d)
    assert got.shape == e_d.shape and got.dtype == torch.complex64 and got.is_cuda and torch.view_as_real(got2).isfinite().all()
    from adafortitran_amd.chansim import frame_keys
    keys, sigma, rho = frame_keys(seed, np.arange(32)), noise_sigma(meta[:, 0]), np.ones(32, dtype=np.float32)
    z, dec, errors, flags = link_observe_host(cfg, keys, ideal, est, sigma, rho, pilots, tau=derived_tau(1))
    elems = flags.any(axis=3)
    assert abs(dev.symbol_error_rate() - host.symbol_error_rate()) * 32 * cfg.data_elements <= elems.sum()
    zb = derived_z_bound(cfg, keys, ideal, sigma, dec, 1)
    y = np.abs(ideal.astype(np.complex128) * _sent(cfg, keys)[2] + _noise(cfg, keys, sigma.astype(np.float64)))
    zb = zb + elems * 2 * y / (cfg.d * np.sqrt(2.0))
    gb = derived_grid_bound(tb, z.astype(np.complex64), tb.indices(meta), data_noise_scale(m))
    rms = lambda a: float(np.sqrt((np.abs(a) ** 2).mean()))  # noqa: E731
    allowed = (rms(zb) + 2.0 ** -24 * rms(z) + rms(gb) + 2.0 ** -24 * np.sqrt(2.0) * rms(want)) / rms(ideal)
    nm = lambda a: float(np.sqrt((np.abs(a - ideal) ** 2).mean() / (np.abs(ideal) ** 2).mean()))  # noqa: E731
    got_h = got.cpu().numpy()
    print(f"sqrt(NMSE) device {nm(got_h):.6f}  cpu {nm(want):.6f}  |difference| {abs(nm(got_h) - nm(want)):.3e}  allowed {allowed:.3e}  "
          f"flagged elements {int(elems.sum())}  symbol-error rate device {dev.symbol_error_rate():.5f} cpu {host.symbol_error_rate():.5f}")
    assert abs(nm(got_h) - nm(want)) <= allowed
    assert nm(got_h) < nm(est)


class _Ls(torch.nn.Module):
    """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call."""

    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.cpu().numpy())).to(self.anchor.device)


def test_a_refined_sweep_at_20_db_has_no_more_bit_errors_than_the_unrefined_one():
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    pack = make_pack(sim, 64, seed=40, snr_db=20)
    loaders = [("SNR_20", ingest.ResidentLoader(pack, sim.pilot, 32, device=DEV, shuffle=False))]
    for name, model in (("LMMSE", LmmseEstimator(sim).to(DEV)), ("LS", _Ls(sim).to(DEV))):
        plain, refined = get_link_stats(model, loaders, cfg, seed=5)[20], get_link_stats(model, loaders, cfg, seed=5, refine=1)[20]
        print(f"{name} at 20 dB, 16-QAM, 64 frames: BER {plain:.5f} -> {refined:.5f} after one pass")
        assert refined <= plain
