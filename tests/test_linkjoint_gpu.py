"""``aft_link_joint_f32``, ``hip_ops.LinkJointPlan`` and ``detector="joint"`` on the accumulators and sweeps on the HIP device: the kernel's
counts, LLRs and losses against the float64 definition (``linksim.link_joint_host``) through the bounds derived below, an unheard second
stream, independence of the batch, of the position and of the run, no unwritten element, the 8- and 4-byte forms, the checked build,
the refusals, the coded accumulators against the host decoders on the device's own LLRs, and the physical orderings beside MMSE.

The shapes are tests/test_linksm.py's ``sm_inputs`` and ``sm_cases``: 16 frames of 120 x 14, 32 of 30 x 7 and the four frames of 3 x 5, R
in (2, 3, 4, 8) on the frames whole groups of 2 R fill, the LMMSE estimate and the channel itself.

The bounds (``test_linkjoint.derived_tau_joint`` / ``derived_e_lambda_joint``) follow the kernel's operation chain (csrc/k_linkjoint.hip,
``link_joint_llrs``) as tests/test_linksm_gpu.py follows its own: u = 2^-24, every float32 operation errs by at most u times its result,
no fast-math, nothing contracted behind the source; ``rho`` and ``scale`` are the same float32 numbers on both sides.  A complex quantity
carries a bound on the MAGNITUDE of its error; its two components then sum to at most sqrt(2) times it.  Every error is written in
units of the SHARE of ``Q = 2 A^2 (g00 + g11 + 2 G01) + 2 sqrt(2) A (reach(m_0) + reach(m_1))`` that bounds the term (``linksim``, "the
joint link"), so the errors of a candidate's terms add up to a multiple of ``Q``:

* the operands, from tests/test_linksm_gpu.py: ``m_s`` within e_m(R) of reach(m_s) (about 34 u at R = 8), ``g00`` / ``g11`` within
  e_g(R) = (1+u)^(2+R) - 1 of themselves and ``g01`` within e_g(R) of G01; a level ``a_k = d (2 k - (L-1))`` within e_a = (1+u)^2 - 1
  (d rounds once, the product once; the integer is exact).
* the stream's own terms, per axis ``t(k) = a_k fma(a_k, g_ee, -2 comp)``: the piece ``a_k^2 g_ee`` carries two levels, the sum and two
  roundings, e_p = (1+e_a)^2 (1+e_g) (1+u)^2 - 1 of ``A^2 g_ee``; the piece ``2 a_k comp`` one level, the component and the same two
  roundings.  Over both axes the components sum to at most sqrt(2) reach(m_e) and their errors to sqrt(2) e_m reach(m_e), so
  e_t = max(e_p, (1+e_a)(1+e_m)(1+u)^2 - 1) of the share ``2 A^2 g_ee + 2 sqrt(2) A reach(m_e)``.
* ``z = m_o - g_oe x_e``, two fused multiply-adds per component (the products exact inside them), whose partial sums stay within
  ``Z = reach(m_o) + sqrt(2) A G01``: e_z = (1 + max(e_m, (1+e_g)(1+e_a) - 1))(1+u)^2 - 1 of Z, as a magnitude.
* the inner minimum, per axis ``min_i fma(-2 a_i, |comp z|, a_i^2 g_oo)`` over the positive levels.  In exact arithmetic it is
  ``min_k mu_k``: the mirrored level's metric is larger by ``4 a_i |comp|``.  ``a_i^2 g_oo = (a_i a_i) g_oo`` is within e_p of ``A^2 g_oo``,
  ``-2 a_i`` is exact in ``a_i``, the fused multiply-add rounds once; a minimum of perturbed metrics moves by at most the largest
  perturbation.  Over both axes: e_r = max((1+e_p)(1+u) - 1, (1+e_a)(1+u)(1+e_z) - 1) of the share ``2 A^2 g_oo + 2 sqrt(2) A Z``
  ``= 2 A^2 g_oo + 2 sqrt(2) A reach(m_o) + 4 A^2 G01``.
* ``f = (t(ki) + t(kq)) + (r_I + r_Q)``: every term passes two additions: e_f(R) = (1 + max(e_t, e_r))(1+u)^2 - 1 of Q, about 41 u at
  R = 8.

A bit's two minima each move by at most e_f Q and their difference rounds once, ``|min1 - min0| <= 2 Q (1 + e_f)``:
tau(R) = 2 e_f + 2 u (1 + e_f), 5.0e-6 at R = 8.  ``Lambda_j = scale Delta_j`` rounds once more: e_lambda(R) = tau + u (2 + tau), 5.2e-6
at R = 8.  Both are below TAU_CAP = 1e-5.  A device decision is the sign of the device's own LLR, so it can differ from the
definition's only on a flagged bit: the counts are compared through the flagged bits and elements of each row, whose shares
tests/test_linkjoint.py caps.  The loss is compared as tests/test_linksoft_gpu.py compares it (``derived_e_s``: the softplus terms and
the order of a stream's sums are the soft kernel's).

Measured on one MI355X (the figures this file prints): see the table in DESIGN.md, "Joint detection on the link"."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, make_pack
from adafortitran_amd.hip_ops import LinkJointPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator,
                                      LdpcConfig, LinkConfig, link_decode_host, link_joint_host, link_ldpc_host, link_mrc_host,
                                      noise_sigma, sm_weights)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linkjoint import JOINT_ELEMENT_SHARE_CAP, derived_e_lambda_joint, derived_tau_joint, joint_flagged_shares
from test_linkmrc import MRC_ODD
from test_linksim import TAU_CAP
from test_linksim_gpu import _dev
from test_linksm import SM_SHARE_CAP, sm_cases, sm_inputs
from test_linksm_gpu import _Ls
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7777
FACTORS = np.asarray(DEFAULT_FACTORS[:3], dtype=np.float32)


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    assert derived_tau_joint(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda_joint(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


_plans, _wants, _ops = {}, {}, {}


def _plan(name, m, R):
    if (name, m, R) not in _plans:
        _plans[name, m, R] = LinkJointPlan(LinkConfig(sm_inputs(name)[0], m), DEV, R)
    return _plans[name, m, R]


def _operands(name, R, which="lmmse"):
    """The frames whole groups of 2 R fill, on the host and on the device: (n, (keys, sigma, rho, scale, ideal, est)) twice."""
    if (name, R, which) not in _ops:
        sim, keys, sigma, snr, ideal, est = sm_inputs(name)
        n = len(keys) // (2 * R) * 2 * R
        rho, scale, _ = sm_weights(snr[:n], 0.0, R, 2)
        host = (keys[:n], sigma[:n], rho, scale, ideal[:n], est[which][:n])
        _ops[name, R, which] = (n, host, tuple(_dev(a) for a in host))
    return _ops[name, R, which]


def _want(name, m, R, which):
    """The definition at tau(R) and e_lambda(R), computed once and flattened to G N rows: (counts, loss, llr, wrong, flags, loss_lo,
    loss_hi, q), and the flags unflattened first."""
    if (name, m, R, which) not in _wants:
        _, (keys, sigma, rho, scale, ideal, est), _ = _operands(name, R, which)
        out = link_joint_host(LinkConfig(sm_inputs(name)[0], m), keys, ideal, est, sigma, rho, scale, R, 2, FACTORS,
                              tau=derived_tau_joint(R), e_lambda=derived_e_lambda_joint(R))
        _wants[name, m, R, which] = (out[4],) + tuple(v.reshape(-1, *v.shape[2:]) for v in out)
    return _wants[name, m, R, which]


def _run(name, m, R, which="lmmse", want_llr=True, lib=None):
    _, _, (k, s, rho, c, h, e) = _operands(name, R, which)
    return _plan(name, m, R)(h, e, k, s, rho, c, _dev(FACTORS), want_llr=want_llr, lib=lib)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    rows = with_flags = differing = 0
    worst_llr = worst_bits = worst_elems = 0.0
    for name, R, n in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        e_s, e_l = derived_e_s(cfg), derived_e_lambda_joint(R)
        for which in ("lmmse", "ideal"):
            flags5, want_counts, _, want_llr, _, flags, lo, hi, q = _want(name, m, R, which)
            counts, loss, llr = _run(name, m, R, which)
            F = n // R                                                         # G N rows
            assert counts.shape == (F, 2) and counts.dtype == torch.int32 and loss.shape == (F, 3) and llr.shape == (F, *cfg.sim.ofdm, m)
            bits, elems = joint_flagged_shares(cfg, flags5)
            assert bits <= SM_SHARE_CAP and elems <= JOINT_ELEMENT_SHARE_CAP, (name, R, which, bits, elems)
            got = counts.cpu().numpy().astype(np.int64)
            flagged_bits, flagged_elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
            assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= flagged_bits).all(), (name, R, which, got, want_counts, flagged_bits)
            assert (np.abs(got[:, 1] - want_counts[:, 1]) <= flagged_elems).all(), (name, R, which, got, want_counts, flagged_elems)
            got_llr = llr.cpu().numpy().astype(np.float64)
            err = np.abs(got_llr - want_llr)
            ratio = float((err[q > 0] / q[q > 0] / e_l).max())
            print(f"m = {m}, {name}, R = {R}, {which}: largest |llr_dev - llr_def| / (e_lambda(R) q) = {ratio:.3f}; flagged shares {bits:.2e} of "
                  f"the bits, {elems:.2e} of the elements; rows that differ {int((got != want_counts).any(axis=1).sum())} of {F}")
            assert np.isfinite(got_llr).all() and (err <= e_l * q).all(), (name, R, which, ratio)
            got_loss = loss.cpu().numpy().astype(np.float64)
            assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                (name, R, which, got_loss, lo, hi)
            rows += F
            with_flags += int((flagged_bits > 0).sum())
            differing += int((got != want_counts).any(axis=1).sum())
            worst_llr, worst_bits, worst_elems = max(worst_llr, ratio), max(worst_bits, bits), max(worst_elems, elems)
    print(f"m = {m}: {with_flags} of {rows} (group, stream) rows had a flagged bit at tau(R); {differing} differ from the definition; largest "
          f"flagged shares {worst_bits:.2e} (bits) and {worst_elems:.2e} (elements); largest |llr_dev - llr_def| / (e_lambda(R) q) = {worst_llr:.3f}")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_stream(m):
    """``H_r1 = E_r1 = 0``: every candidate of stream 1 has the same metric, so its LLRs are exactly 0 on the device; stream 0's are
    within e_lambda(R) q of ``link_mrc_host``'s on the frames (r, 0), which the definition equals there."""
    f = _dev(FACTORS)
    for name, R, _ in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        n, (keys, sigma, rho, scale, ideal, est), _ = _operands(name, R)
        G = n // (2 * R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        counts, loss, llr = _plan(name, m, R)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale)), f, want_llr=True)
        llr = llr.view(G, 2, *llr.shape[1:])
        assert (llr[:, 1] == 0).all(), (name, R)
        q = link_joint_host(cfg, keys, H, E, sigma, rho, scale, R, e_lambda=0.0)[5]
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R)[2]
        err = np.abs(llr[:, 0].cpu().numpy().astype(np.float64) - want)
        assert (err <= derived_e_lambda_joint(R) * q[:, 0]).all(), (name, R, float((err / np.where(q[:, 0] > 0, q[:, 0], 1)).max()))
        np.testing.assert_allclose(loss.view(G, 2, -1)[:, 1, 0].cpu().numpy(), m * cfg.data_elements, rtol=1e-5)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, snr, ideal, est = sm_inputs(name)
        for R in (2, 3):
            plan, W = _plan(name, m, R), 2 * R
            idx = (np.arange(37 * W) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-W:] = np.arange(W, 2 * W)                                       # ... the last one group 1 of ``_operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est["lmmse"][i]), _dev(keys[i]), _dev(sigma[i]),  # noqa: E731
                             *(_dev(a) for a in sm_weights(snr[i], 0.0, R, 2)[:2]))
            batch = plan(*ops(idx), f, want_llr=True)
            alone = plan(*ops(np.arange(W, 2 * W)), f, want_llr=True)
            _same_bits([t[72:74] for t in batch], alone)
            _same_bits([t[2:4] for t in _run(name, m, R)], alone)                # second of the groups of ``_operands``
            _same_bits(plan(*ops(idx), f, want_llr=True), batch)                 # a second run of the same batch


def _entry(plan, ops, factors, counts, loss, llr, batch, hp=None, ep=None, lib=None):
    lib = lib or _lib.load()
    k, s, rho, c, h, e = ops
    return lib.aft_link_joint_f32(ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), k.data_ptr(), s.data_ptr(),
                                  rho.data_ptr(), c.data_ptr(), factors.data_ptr(), factors.numel(), plan.branches, plan.streams,
                                  counts.data_ptr(), loss.data_ptr(), llr, batch, _lib.current_stream_ptr(counts.device))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m):
    """Every element of the three outputs is written and nothing beside them; without the LLR output, and with ideal, est and llr 8, 4
    and 12 bytes off a 16-byte boundary (the 8-byte loads, the 8- and 4-byte stores), the same bits."""
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        for R in (2, 3):
            n, _, ops = _operands(name, R)
            plan, F = _plan(name, m, R), n // R
            want = _run(name, m, R)
            h, e = ops[4], ops[5]
            fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
            fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
            assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
            for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (None, fe.data_ptr() + 8, 0), (None, None, 8),
                                (None, None, 4), (fh.data_ptr() + 8, None, 12), (None, None, None)):
                counts = torch.full((F + 1, 2), POISON, dtype=torch.int32, device=DEV)
                loss = torch.full((F + 1, 3), float("nan"), device=DEV)
                llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
                _lib.check(_entry(plan, ops, f, counts, loss, None if off is None else llr.data_ptr() + off, n, hp, ep))
                _same_bits([counts[:F], loss[:F]], want[:2])
                assert (counts[F:] == POISON).all() and loss[F:].isnan().all()
                if off is None:
                    assert llr.isnan().all()
                else:
                    at = off // 4
                    _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                    assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
            _same_bits(_run(name, m, R, want_llr=False)[:2], want[:2])
    # the odd grid whose last element (14, at (2, 4)) is data and alone in its pair: written for both streams, finite and not a pilot's zero
    n, _, ops = _operands(MRC_ODD, 2)
    counts = torch.full((2, 2), POISON, dtype=torch.int32, device=DEV)
    loss, llr = torch.full((2, 3), float("nan"), device=DEV), torch.full((2, 3, 5, m), float("nan"), device=DEV)
    _lib.check(_entry(_plan(MRC_ODD, m, 2), ops, f, counts, loss, llr.data_ptr(), n))
    _same_bits([counts, loss, llr], _run(MRC_ODD, m, 2))
    assert llr.isfinite().all() and (llr[:, 2, 4] != 0).all() and (llr[:, 1, 2] == 0).all()


def test_all_zero_estimates_give_zero_llrs():
    for m in BITS_PER_SYMBOL:
        _, _, (k, s, rho, c, h, e) = _operands("odd_30x7", 2)
        counts, loss, llr = _plan("odd_30x7", m, 2)(h, torch.zeros_like(e), k, s, rho, c, _dev(FACTORS), want_llr=True)
        assert (llr == 0).all() and loss.isfinite().all() and (counts >= 0).all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_joint_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_joint_f32")
    for name in ("default_120x14", "odd_30x7"):
        for m in BITS_PER_SYMBOL:
            for R in (2, 3, 8):
                _same_bits(_run(name, m, R, lib=lib), _run(name, m, R))
    for m in BITS_PER_SYMBOL:
        _same_bits(_run(MRC_ODD, m, 2, lib=lib), _run(MRC_ODD, m, 2))


def test_what_the_plan_refuses():
    n, _, (k, s, rho, c, h, e) = _operands("odd_30x7", 4)
    plan, f = _plan("odd_30x7", 4, 4), _dev(FACTORS)
    for args, word in (((h[:6], e[:6], k[:6], s[:6], rho[:6], c, f), "6 frames is not a multiple of branches \\* streams = 4 \\* 2"),
                       ((h, e, k, s, rho[:8], c, f), "rho must hold"), ((h, e, k, s, rho, c[:3], f), "scale must hold"),
                       ((h, e, k, s, rho, c.double(), f), "scale must be torch.float32"),
                       ((h, e, k, s, rho, torch.from_numpy(np.zeros(4, np.float32)), f), "pinned host memory"),
                       ((h, e, k, s, rho, c, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    for bad in (0, 1, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkJointPlan(plan.cfg, DEV, bad)
    for bad in (1, 3, 2.0, True):
        with pytest.raises(ValueError, match="streams"):
            LinkJointPlan(plan.cfg, DEV, 2, bad)
    with pytest.raises(ValueError, match="LinkJointPlan runs on a HIP device"):
        LinkJointPlan(plan.cfg, "cpu", 2)


def test_every_refusal_of_the_entry_point_launches_nothing():
    name, m, R = "default_120x14", 4, 2
    n, _, (k, s, rho, c, h, e) = _operands(name, R)
    lib, F, f = _lib.load(), n // R, _dev(FACTORS)
    cfg = LinkConfig(sm_inputs(name)[0], m)
    counts = torch.full((F, 2), POISON, dtype=torch.int32, device=DEV)
    loss = torch.full((F, 3), float("nan"), device=DEV)
    llr = torch.full((F, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), rho=rho.data_ptr(), scale=c.data_ptr(),
                factors=f.data_ptr(), n_factors=3, branches=R, streams=2, counts=counts.data_ptr(), loss=loss.data_ptr(),
                llr=llr.data_ptr(), batch=n)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return lib.aft_link_joint_f32(ctypes.byref(p), *(a[x] for x in good), None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_joint_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
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
    for bad in (1, 3, 0, -2):
        refused(SH, f"streams = {bad}", streams=bad)
    for bad in (1, 0, 9, -2):
        refused(SH, f"branches = {bad} is outside 2..8", branches=bad)
    refused(E, "batch = 16 is not a multiple of branches * streams = 3 * 2", branches=3)
    refused(E, "batch = 14 is not a multiple of branches * streams = 2 * 2", batch=14)

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
    assert call(one, batch=4) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert counts[:2].tolist() == [[0, 0]] * 2 and loss[:2].tolist() == [[0.0] * 3] * 2 and llr.reshape(-1)[:2 * m].tolist() == [0.0] * (2 * m)


@pytest.mark.parametrize("kind", ("viterbi", "ldpc"))
def test_coded_accumulators_with_the_joint_detector_run_without_a_synchronisation(kind):
    R, N, seed = 2, 2, 2
    sim = ChannelSimConfig()
    link = LinkConfig(sim, 4)
    code = CodeConfig(link, 256, "3/4") if kind == "viterbi" else LdpcConfig(link, "1/2")
    make = BlockErrorAccumulator if kind == "viterbi" else LdpcBlockErrorAccumulator
    decode = link_decode_host if kind == "viterbi" else link_ldpc_host
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    with_est, perfect, on_device = (make(code, DEV, seed=seed, branches=R, streams=N, detector="joint") for _ in range(3))
    assert isinstance(with_est._plan, LinkJointPlan)
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
    rows = 48 // R                                # G N
    assert len(seen) == 3 and with_est.frames == perfect.frames == rows and with_est.errors.is_cuda and with_est.errors.dtype == torch.int64
    # what the accumulator launched, step by step: the detector's LLRs through the host decoder, with the keys of frames (0, s)
    plan, one = LinkJointPlan(link, DEV, R), torch.ones(1, device=DEV)
    want = np.zeros((2, len(with_est.errors)), np.int64)
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        sent_keys = np.ascontiguousarray(keys.reshape(-1, R, N)[:, 0, :]).reshape(-1)
        rho, scale, _ = sm_weights(snr, 0.0, R, N)
        for i, e in enumerate((est, ideal)):
            _, _, llr = plan(ideal, e, _dev(keys), _dev(noise_sigma(snr)), _dev(rho), _dev(scale), one, want_llr=True)
            want[i] += decode(code, sent_keys, llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()     # keys hashed on the device are the host's
    assert with_est.result() == want[0][1] / (rows * code.blocks) and perfect.result() <= with_est.result()
    print(f"{kind}, 2 x 2 joint: BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}")


def test_physical_orderings_on_the_device():
    """Recorded and printed; asserted is the ordering only.  One simulated pack of 64 frames at 15 dB, 16-QAM."""
    from adafortitran_amd.evaluation import get_link_rates, get_link_stats
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    pack = make_pack(sim, 64, seed=31, snr_db=15.0)
    loaders = [("SNR_15", ingest.ResidentLoader(pack, sim.pilot, 32, device=DEV, shuffle=False))]
    models = {"perfect": None, "lmmse": LmmseEstimator(sim).to(DEV), "ls": _Ls(sim).to(DEV)}
    ber = {(R, d): {name: get_link_stats(model, loaders, cfg, seed=1, branches=R, streams=2, detector=d)[15] for name, model in models.items()}
           for R in (2, 4, 8) for d in ("mmse", "joint")}
    gmi = {(R, d): {name: get_link_rates(models[name], loaders, cfg, seed=1, branches=R, streams=2, detector=d)[15] for name in ("perfect", "lmmse")}
           for R in (2, 8) for d in ("mmse", "joint")}
    print("BER per (antennas, detector) and estimator:", ber, " GMI per stream:", gmi)
    print("LS, joint against MMSE:", {R: (ber[R, "joint"]["ls"], ber[R, "mmse"]["ls"]) for R in (2, 4, 8)},
          " R = 8, joint against MMSE:", {w: (ber[8, "joint"][w], ber[8, "mmse"][w]) for w in models})
    for w in ("perfect", "lmmse"):
        assert ber[2, "joint"][w] <= ber[2, "mmse"][w] and gmi[2, "joint"][w] >= gmi[2, "mmse"][w]
    assert all(ber[2, "joint"][w] > ber[4, "joint"][w] > ber[8, "joint"][w] for w in models)           # BER falls with R
    assert all(ber[R, "joint"]["perfect"] <= ber[R, "joint"]["lmmse"] <= ber[R, "joint"]["ls"] for R in (2, 4, 8))
