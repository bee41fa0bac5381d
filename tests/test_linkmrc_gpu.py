"""``aft_link_mrc_f32``, ``hip_ops.LinkMrcPlan`` and the ``branches=`` argument of the accumulators and sweeps on the HIP device: the
kernel's counts, LLRs and losses against the float64 definition (``linksim.link_mrc_host``) through the bounds derived below, one branch
against the single-branch kernels bit for bit, independence of the batch, of the position and of the run, no unwritten element, the
8- and 4-byte forms, the checked build, the entry point's refusals, the coded accumulators against the host decoders on the device's
own LLRs, and the physical orderings.

The shapes are tests/test_linkmrc.py's ``mrc_inputs``: seed 3, frames 0..7 of the default grid (16-byte loads, 840 pairs over 256
threads) and 0..15 of 30 x 7 (odd T: 8-byte loads, a ragged last pass), each frame at the SNR it was drawn with, so the weights are
mixed (``rho`` reaches 316); R in (1, 2, 3, 4, 8), R = 3 on the first 6 and 15 frames.  With R = 1 and 2 also the two frames of 3 x 5
(``MRC_ODD``: an odd number of elements whose last is data, alone in its pair).

The bounds extend tests/test_linksim_gpu.py's ``derived_tau`` and tests/test_linksoft_gpu.py's ``derived_e_lambda`` to R branches, in
units of the summed reach ``sum_r rho_r (|H_r||x| + |noise_r|) |E_r|`` (u = 2^-24, no fast-math; ``rho`` and ``scale`` are the same
float32 numbers on both sides):

* a branch's c_r is the single-branch kernel's: within e_c1 = ``test_linksim_gpu.derived_tau()`` (about 29 u) of its own reach.
* c = fma(rho_r, c_r, c): the product is exact inside the fused multiply-add and the partial sum rounds once.  Every partial sum is
  at most (1 + e) times the partial reach, so R branches give  e_c(R) = (1 + e_c1)(1 + u)^R - 1  of the summed reach.
* p_r = fma(E_re, E_re, E_im E_im) is a sum of non-negative terms rounded twice and p = fma(rho_r, p_r, p) rounds once per branch,
  all terms non-negative:  e_p(R) = (1 + u)^(2 + R) - 1.
* beta_b p: 2 d is float32's rounding of the exact value, the product with p rounds, the product with the integer rounds:
  e_t(R) = (1 + u)^(5 + R) - 1.

tau(R) = max(e_c(R), e_t(R)): 2.2e-6 at R = 8.  e_lambda(R) is ``derived_e_lambda`` with e_c = tau(R) and e_p = e_p(R): 5.5e-6 at
R = 8.  Both are below TAU_CAP = 1e-5, so AFT_LINK_MAX_BRANCHES stays 8.  The loss is compared as tests/test_linksoft_gpu.py compares
it (``derived_e_s``: the softplus terms and the order of the sums are the soft kernel's)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, make_pack
from adafortitran_amd.hip_ops import LinkMrcPlan, LinkPlan, LinkSoftPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator,
                                      LdpcConfig, LinkConfig, branch_weights, link_decode_host, link_ldpc_host, link_mrc_host,
                                      llr_scale, noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linkmrc import MRC_GRIDS, MRC_ODD, mrc_inputs
from test_linksim import SHARE_CAP, TAU_CAP, flagged_share
from test_linksim_gpu import U, _dev, derived_tau as derived_tau_1
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7777
FACTORS = np.asarray(DEFAULT_FACTORS[:3], dtype=np.float32)
BRANCHES = (1, 2, 3, 4, 8)
#: every grid with the branches its frames allow: the odd grid whose last element is data has two frames
CASES = tuple((name, BRANCHES) for name in MRC_GRIDS) + ((MRC_ODD, (1, 2)),)


def derived_tau(R: int) -> float:
    e_c = (1 + derived_tau_1()) * (1 + U) ** R - 1
    e_t = (1 + U) ** (5 + R) - 1
    return float(max(e_c, e_t))


def derived_e_lambda(R: int) -> float:
    e_c = derived_tau(R)
    e_a, e_p = (1 + U) ** 2 - 1, (1 + U) ** (2 + R) - 1
    e_i = max((1 + e_a) * (1 + e_p), 1 + e_c) * (1 + U) - 1
    e_mu = (1 + e_a) * (1 + U) * (1 + e_i) - 1
    e_d = 2 * e_mu + 2 * U * (1 + e_mu)
    return float(e_d + U * (2 + e_d))


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    for R in BRANCHES:
        print(f"R = {R}: tau = {derived_tau(R):.3e} = {derived_tau(R) / U:.1f} u, e_lambda = {derived_e_lambda(R):.3e} = "
              f"{derived_e_lambda(R) / U:.1f} u")
    assert derived_tau_1() < derived_tau(1) < derived_tau(2) < derived_tau(8) <= derived_tau_1() + 9 * U
    assert derived_tau(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


_plans, _wants, _ops = {}, {}, {}


def _plan(name, m, R):
    if (name, m, R) not in _plans:
        _plans[name, m, R] = LinkMrcPlan(LinkConfig(mrc_inputs(name)[0], m), DEV, R)
    return _plans[name, m, R]


def _operands(name, R, which="lmmse"):
    """The frames R divides, on the host and on the device: (n, keys, sigma, rho, scale, ideal, est) twice."""
    if (name, R, which) not in _ops:
        sim, keys, sigma, snr, ideal, est = mrc_inputs(name)
        n = len(keys) // R * R
        rho, scale = branch_weights(snr[:n], 0.0, R)
        host = (keys[:n], sigma[:n], rho, scale, ideal[:n], est[which][:n])
        _ops[name, R, which] = (n, host, tuple(_dev(a) for a in host))
    return _ops[name, R, which]


def _want(name, m, R, which):
    """The definition at tau(R) and e_lambda(R), computed once: (counts, loss, llr, wrong, flags, loss_lo, loss_hi, q)."""
    if (name, m, R, which) not in _wants:
        _, (keys, sigma, rho, scale, ideal, est), _ = _operands(name, R, which)
        _wants[name, m, R, which] = link_mrc_host(LinkConfig(mrc_inputs(name)[0], m), keys, ideal, est, sigma, rho, scale, R, FACTORS,
                                                  tau=derived_tau(R), e_lambda=derived_e_lambda(R))
    return _wants[name, m, R, which]


def _run(name, m, R, which="lmmse", want_llr=True, lib=None):
    _, _, (k, s, rho, c, h, e) = _operands(name, R, which)
    return _plan(name, m, R)(h, e, k, s, rho, c, _dev(FACTORS), want_llr=want_llr, lib=lib)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    groups = with_flags = differing = 0
    worst_llr = 0.0
    for name, branches in CASES:
        cfg = LinkConfig(mrc_inputs(name)[0], m)
        e_s = derived_e_s(cfg)
        for R in branches:
            for which in ("lmmse", "ideal"):
                want_counts, _, want_llr, _, flags, lo, hi, q = _want(name, m, R, which)
                counts, loss, llr = _run(name, m, R, which)
                G = _operands(name, R, which)[0] // R
                assert counts.shape == (G, 2) and counts.dtype == torch.int32 and loss.shape == (G, 3) and llr.shape == (G, *cfg.sim.ofdm, m)
                assert flagged_share(cfg, flags) <= SHARE_CAP
                got = counts.cpu().numpy().astype(np.int64)
                pairs, elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
                assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= pairs).all(), (name, R, which, got, want_counts, pairs)
                assert (np.abs(got[:, 1] - want_counts[:, 1]) <= elems).all(), (name, R, which, got, want_counts, elems)
                got_llr = llr.cpu().numpy().astype(np.float64)
                err = np.abs(got_llr - want_llr)
                assert np.isfinite(got_llr).all() and (err <= derived_e_lambda(R) * q).all(), (name, R, which, float((err / np.where(q > 0, q, 1)).max()))
                got_loss = loss.cpu().numpy().astype(np.float64)
                assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                    (name, R, which, got_loss, lo, hi)
                groups += G
                with_flags += int((pairs > 0).sum())
                differing += int((got != want_counts).any(axis=1).sum())
                worst_llr = max(worst_llr, float((err[q > 0] / q[q > 0] / derived_e_lambda(R)).max()))
    print(f"m = {m}: {with_flags} of {groups} groups had a flagged decision at tau(R); {differing} differ from the definition; "
          f"largest |llr_dev - llr_def| / (e_lambda(R) q) = {worst_llr:.2f}")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_one_branch_is_the_single_branch_kernels_bit_for_bit(m):
    for name, _ in CASES:
        cfg = LinkConfig(mrc_inputs(name)[0], m)
        hard, soft = LinkPlan(cfg, DEV), LinkSoftPlan(cfg, DEV)
        for which in ("lmmse", "ideal"):
            _, _, (k, s, rho, c, h, e) = _operands(name, 1, which)
            assert (rho == 1).all()
            counts, loss, llr = _run(name, m, 1, which)
            want_loss, want_llr = soft(h, e, k, s, c, _dev(FACTORS), want_llr=True)
            assert torch.equal(counts, hard(h, e, k, s)) and torch.equal(loss, want_loss) and torch.equal(llr, want_llr)
            _same_bits([loss, llr], [want_loss, want_llr])                       # the sums start at -0: the sign of a zero, too
    # the odd grid whose last element (14, at (2, 4)) is data and alone in its pair: written by both kernels into a poisoned LLR
    # output, finite and not a pilot's zero, with one branch and with two; without it the counts of -H would read (26, 13)
    cfg = LinkConfig(mrc_inputs(MRC_ODD)[0], m)
    f = _dev(FACTORS)
    for R in (1, 2):
        n, _, ops = _operands(MRC_ODD, R)
        G = n // R
        counts = torch.full((G, 2), POISON, dtype=torch.int32, device=DEV)
        loss, llr = torch.full((G, 3), float("nan"), device=DEV), torch.full((G, 3, 5, m), float("nan"), device=DEV)
        _lib.check(_entry(_plan(MRC_ODD, m, R), ops, f, counts, loss, llr.data_ptr(), n))
        _same_bits([counts, loss, llr], _run(MRC_ODD, m, R))
        assert llr.isfinite().all() and (llr[:, 2, 4] != 0).all() and (llr[:, 1, 2] == 0).all()
        k, s, rho, c, h, e = ops
        zero = torch.zeros_like(s)
        assert _plan(MRC_ODD, m, R)(h, -h, k, zero, rho, c, f)[0].tolist() == [[28, 14]] * G
    k, s, rho, c, h, e = _operands(MRC_ODD, 1)[2]
    soft_llr = torch.full((2, 3, 5, m), float("nan"), device=DEV)
    soft_loss = torch.full((2, 3), float("nan"), device=DEV)
    _lib.check(_lib.load().aft_link_soft_f32(ctypes.byref(cfg.to_struct()), h.data_ptr(), e.data_ptr(), k.data_ptr(), s.data_ptr(), c.data_ptr(),
                                             f.data_ptr(), 3, soft_loss.data_ptr(), soft_llr.data_ptr(), 2, _lib.current_stream_ptr(h.device)))
    _same_bits([soft_loss, soft_llr], _run(MRC_ODD, m, 1)[1:])
    assert soft_llr.isfinite().all() and (soft_llr[:, 2, 4] != 0).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    for name in MRC_GRIDS:
        sim, keys, sigma, snr, ideal, est = mrc_inputs(name)
        f = _dev(FACTORS)
        for R in (2, 3):
            plan = _plan(name, m, R)
            idx = (np.arange(37 * R) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-R:] = np.arange(R, 2 * R)                                       # ... the last one group 1 of ``_operands``
            rho, scale = branch_weights(snr[idx], 0.0, R)
            batch = plan(_dev(ideal[idx]), _dev(est["lmmse"][idx]), _dev(keys[idx]), _dev(sigma[idx]), _dev(rho), _dev(scale), f, want_llr=True)
            rho1, scale1 = branch_weights(snr[R:2 * R], 0.0, R)
            alone = plan(_dev(ideal[R:2 * R]), _dev(est["lmmse"][R:2 * R]), _dev(keys[R:2 * R]), _dev(sigma[R:2 * R]), _dev(rho1), _dev(scale1),
                         f, want_llr=True)
            _same_bits([t[36:37] for t in batch], alone)
            _same_bits([t[1:2] for t in _run(name, m, R)], alone)                # second of the groups of ``_operands``
            _same_bits(plan(_dev(ideal[idx]), _dev(est["lmmse"][idx]), _dev(keys[idx]), _dev(sigma[idx]), _dev(rho), _dev(scale), f,
                            want_llr=True), batch)                               # a second run of the same batch


def _entry(plan, ops, factors, counts, loss, llr, batch, hp=None, ep=None, lib=None):
    lib = lib or _lib.load()
    k, s, rho, c, h, e = ops
    return lib.aft_link_mrc_f32(ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), k.data_ptr(), s.data_ptr(), rho.data_ptr(),
                                c.data_ptr(), factors.data_ptr(), factors.numel(), plan.branches, counts.data_ptr(),
                                loss.data_ptr(), llr, batch, _lib.current_stream_ptr(counts.device))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m):
    """Every element of the three outputs is written and nothing beside them; without the LLR output, and with ideal, est and llr 8, 4
    and 12 bytes off a 16-byte boundary (the 8-byte loads, the 8- and 4-byte stores), the same bits."""
    f = _dev(FACTORS)
    for name in MRC_GRIDS:
        for R in (2, 3):
            n, _, ops = _operands(name, R)
            plan, G = _plan(name, m, R), n // R
            want = _run(name, m, R)
            h, e = ops[4], ops[5]
            fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
            fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
            assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
            for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (None, fe.data_ptr() + 8, 0), (None, None, 8),
                                (None, None, 4), (fh.data_ptr() + 8, None, 12), (None, None, None)):
                counts = torch.full((G + 1, 2), POISON, dtype=torch.int32, device=DEV)
                loss = torch.full((G + 1, 3), float("nan"), device=DEV)
                llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
                _lib.check(_entry(plan, ops, f, counts, loss, None if off is None else llr.data_ptr() + off, n, hp, ep))
                _same_bits([counts[:G], loss[:G]], want[:2])
                assert (counts[G:] == POISON).all() and loss[G:].isnan().all()
                if off is None:
                    assert llr.isnan().all()
                else:
                    at = off // 4
                    _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                    assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
            _same_bits(_run(name, m, R, want_llr=False)[:2], want[:2])


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_mrc_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_mrc_f32")
    for name in MRC_GRIDS:
        for m in BITS_PER_SYMBOL:
            for R in (1, 3, 8):
                _same_bits(_run(name, m, R, lib=lib), _run(name, m, R))
    for m in BITS_PER_SYMBOL:
        _same_bits(_run(MRC_ODD, m, 2, lib=lib), _run(MRC_ODD, m, 2))


def test_what_the_plan_refuses():
    n, _, (k, s, rho, c, h, e) = _operands("odd_30x7", 4)
    plan, f = _plan("odd_30x7", 4, 4), _dev(FACTORS)
    for args, word in (((h[:6], e[:6], k[:6], s[:6], rho[:6], c, f), "6 frames is not a multiple of branches = 4"),
                       ((h, e, k, s, rho[:8], c, f), "rho must hold"), ((h, e, k, s, rho, c[:3], f), "scale must hold"),
                       ((h, e, k, s, rho.double(), c, f), "rho must be torch.float32"),
                       ((h, e, k, s, torch.from_numpy(np.ones(n, np.float32)), c, f), "pinned host memory"),
                       ((h, e, k, s, rho, c, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkMrcPlan(plan.cfg, DEV, bad)
    with pytest.raises(ValueError, match="LinkMrcPlan runs on a HIP device"):
        LinkMrcPlan(plan.cfg, "cpu", 2)


def test_every_refusal_of_the_entry_point_launches_nothing():
    name, m, R = "default_120x14", 4, 2
    n, _, (k, s, rho, c, h, e) = _operands(name, R)
    lib, G, f = _lib.load(), n // R, _dev(FACTORS)
    cfg = LinkConfig(mrc_inputs(name)[0], m)
    counts = torch.full((G, 2), POISON, dtype=torch.int32, device=DEV)
    loss = torch.full((G, 3), float("nan"), device=DEV)
    llr = torch.full((G, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), rho=rho.data_ptr(), scale=c.data_ptr(),
                factors=f.data_ptr(), n_factors=3, branches=R, counts=counts.data_ptr(), loss=loss.data_ptr(), llr=llr.data_ptr(), batch=n)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return lib.aft_link_mrc_f32(ctypes.byref(p), *(a[x] for x in good), None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_mrc_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for x in ("ideal", "est", "keys", "sigma", "rho", "scale", "factors", "counts", "loss"):
        refused(E, "NULL pointer", **{x: None})
    for x in ("ideal", "est", "keys"):
        refused(E, "8-byte", **{x: good[x] + 4})
    for x in ("sigma", "rho", "scale", "factors", "counts", "loss", "llr"):
        refused(E, "4-byte", **{x: good[x] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for nf in (0, 9, -1):
        refused(E, f"n_factors = {nf} is outside 1..8", n_factors=nf)
    for bad in (0, 9, -2):
        refused(SH, f"branches = {bad} is outside 1..8", branches=bad)
    refused(E, "batch = 8 is not a multiple of branches = 3", branches=3)
    refused(E, "batch = 7 is not a multiple of branches = 2", batch=7)

    def struct(**fields):
        p = cfg.to_struct()
        for x, value in fields.items():
            if isinstance(value, tuple):
                getattr(p, x)[value[0]] = value[1]
            else:
                setattr(p, x, value)
        return p

    for fields, word in ((dict(num_scs=0), "num_scs = 0"), (dict(num_symbols=-1), "num_symbols = -1"),
                         (dict(num_scs=1 << 16, num_symbols=(1 << 15) + 1), "more than 2^31 elements"),
                         (dict(pilot_scs=65), "pilot_scs = 65 is outside 1..64"), (dict(pilot_symbols=0), "pilot_symbols = 0"),
                         (dict(num_symbols=1), "larger than the ofdm grid"), (dict(pilot_sc_index=(1, 5)), "pilot_sc_index[1] = 5"),
                         (dict(pilot_sc_index=(11, 120)), "pilot_sc_index[11] = 120"), (dict(pilot_symbol_index=(1, 3)), "strictly increasing"),
                         (dict(bits_per_symbol=0), "bits_per_symbol = 0"), (dict(bits_per_symbol=3), "bits_per_symbol = 3"),
                         (dict(bits_per_symbol=10), "bits_per_symbol = 10")):
        refused(SH, word, p=struct(**fields))
    torch.cuda.synchronize()
    assert (counts == POISON).all() and loss.isnan().all() and llr.isnan().all()     # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    _same_bits([counts, loss, llr], _run(name, m, R))                                # ... and the good call writes it all
    # a grid whose every element is a pilot is legal: counts 0, loss 0, LLR 0
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    assert call(one, batch=2) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert counts[0].tolist() == [0, 0] and loss[0].tolist() == [0.0] * 3 and llr.reshape(-1)[:m].tolist() == [0.0] * m


@pytest.mark.parametrize("kind", ("viterbi", "ldpc"))
def test_coded_accumulators_with_two_branches_run_without_a_synchronisation(kind):
    R, seed = 2, 2
    sim = ChannelSimConfig()
    link = LinkConfig(sim, 4)
    code = CodeConfig(link, 256, "3/4") if kind == "viterbi" else LdpcConfig(link, "1/2")
    make = BlockErrorAccumulator if kind == "viterbi" else LdpcBlockErrorAccumulator
    decode = link_decode_host if kind == "viterbi" else link_ldpc_host
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    with_est, perfect, on_device = (make(code, DEV, seed=seed, branches=R) for _ in range(3))
    it = iter(loader)
    first = next(it)
    seen = []

    def step(batch):
        pil, ideal, meta = batch
        est = model(pil, meta)
        with_est.update(est, ideal, meta)
        perfect.update(None, ideal, meta)
        on_device.update(est, ideal, frame_ids=meta[0].to(DEV, non_blocking=True), snr_db=meta[1])
        seen.append((ideal, est, meta))

    step(first)                                   # the first batch builds the plans and the pinned blocks: outside the guard
    torch.cuda.synchronize()
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                          # the mode is honoured: what follows is not vacuous
        for batch in it:
            step(batch)
    groups = 48 // R
    assert len(seen) == 3 and with_est.frames == perfect.frames == groups and with_est.errors.is_cuda and with_est.errors.dtype == torch.int64
    # what the accumulator launched, step by step: the combiner's LLRs through the host decoder, with the leaders' keys
    plan, one = LinkMrcPlan(link, DEV, R), torch.ones(1, device=DEV)
    want = np.zeros((2, len(with_est.errors)), np.int64)
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        rho, scale = branch_weights(snr, 0.0, R)
        for i, e in enumerate((est, ideal)):
            _, _, llr = plan(ideal, e, _dev(keys), _dev(noise_sigma(snr)), _dev(rho), _dev(scale), one, want_llr=True)
            want[i] += decode(code, keys[::R], llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()     # keys hashed on the device are the host's
    assert with_est.result() == want[0][1] / (groups * code.blocks) and perfect.result() <= with_est.result()
    print(f"{kind}, two branches: BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}")


class _Ls(torch.nn.Module):
    """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call."""

    def __init__(self, sim):
        super().__init__()
        self.sim = sim
        self.register_buffer("anchor", torch.zeros(1))

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.cpu().numpy())).to(pilots.device)


def test_physical_sanity_diversity_removes_errors_and_the_estimators_keep_their_order():
    """Recorded and printed; asserted is the ordering only.  One simulated pack of 64 frames at 15 dB, 16-QAM."""
    from adafortitran_amd.evaluation import get_link_rates, get_link_stats
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    pack = make_pack(sim, 64, seed=31, snr_db=15.0)
    loaders = [("SNR_15", ingest.ResidentLoader(pack, sim.pilot, 32, device=DEV, shuffle=False))]
    models = {"perfect": None, "lmmse": LmmseEstimator(sim).to(DEV), "ls": _Ls(sim).to(DEV)}
    ber = {R: {name: get_link_stats(model, loaders, cfg, seed=1, branches=R)[15] for name, model in models.items()} for R in (1, 2, 4)}
    gmi = {R: get_link_rates(None, loaders, cfg, seed=1, branches=R)[15] for R in (1, 2, 4)}
    print("BER per branches and estimator:", ber, " GMI with the channel:", gmi)
    assert ber[1]["perfect"] > ber[2]["perfect"] > ber[4]["perfect"]
    assert all(ber[R]["perfect"] <= ber[R]["lmmse"] <= ber[R]["ls"] for R in ber)
    assert gmi[1] <= gmi[2] <= gmi[4] <= 4
