"""``aft_link_alamouti_f32``, ``hip_ops.LinkAlamoutiPlan`` and the ``tx_diversity=`` argument of the accumulators on the HIP device: the
kernel's counts, LLRs and losses against the float64 definition (``linksim.link_alamouti_host``) through the bounds derived below, an
unheard second antenna against the diversity kernel bit for bit, independence of the batch, of the position and of the run, no
unwritten element, bases off 16 bytes, the checked build, the refusals, and the coded accumulators against the host decoders on the
device's own LLRs.

The shapes are tests/test_linkalamouti.py's ``al_inputs``: seed 3, frames 0..15 of the default grid (840 (line, slot) indices over 256
threads in both pairings), 0..31 of 30 x 7 (odd lines in both pairings: lone elements; a ragged last pass), the four frames of 3 x 5
(a pilot in the middle; the last element is lone in both pairings) and 0..15 of 9 x 6 with pilot rows 0, 2, 3, 8 and pilot columns
0, 2, 5 (lines that begin and end with a pilot, pairs across one and across two adjacent pilots), each frame at the SNR it was drawn
with, so the weights are mixed; R in (1, 2, 3, 4, 8) on the frames whole groups of 2 R fill; both pairings; the LMMSE estimate and the
channel itself.

The bounds follow the kernel's operation chain as tests/test_linksm_gpu.py follows its own (u = 2^-24, every float32 operation errs by
at most u times its result, no fast-math; ``rho`` and ``scale`` are the same float32 numbers on both sides).  Complex quantities carry
a bound on the MAGNITUDE of their error, which also bounds each component:

* x, H x and the noise as there: e_x = (1+u)^2 - 1, e_h = (1 + e_x)(1 + u)^2 - 1 of |H||x|, the radius within e_r, the unit vector
  within sqrt(2) 8 u: e_n = e_r + sqrt(2) 8 u (1 + e_r) of |noise|.  Negating and conjugating a sent symbol is exact.
* the sample is ``link_sample2``'s: antenna 0's product, antenna 1's two products by one fused multiply-add each, the noise by one
  more: e_y = (1 + max(e_h, e_n))(1 + u)^3 - 1 (about 24 u) of reach(y_r[e]) = |H_r0||t0| + |H_r1||t1| + |noise|.
* a term y conj(E) (or its conjugate, or its negative: exact) is a product and a fused multiply-add per component:
  e_c1 = e_y + 2 u (1 + e_y) of reach(y) |E|.
* a sum c takes two terms per antenna, each by one fused multiply-add whose product is exact inside it: 2 R roundings of partial sums
  that are within the partial reach: e_c(R) = (1 + e_c1)(1 + u)^(2 R) - 1 (about 42 u at R = 8) of reach(c), the combiner's sum with
  every factor replaced by its absolute value.
* p is a sum of non-negative terms |E|^2, each rounded twice, by 2 R fused multiply-adds: e_p(R) = (1 + u)^(2 + 2 R) - 1; the
  threshold beta_b p adds the three roundings of tests/test_linksim_gpu.py (2 d, the product with p, the product with the integer).

tau(R) = max(e_c(R), (1 + e_p(R))(1 + u)^3 - 1): 2.5e-6 at R = 8.  e_lambda(R) is tests/test_linksoft_gpu.py's chain with e_c(R) and
e_p(R) in place of its e_c and e_p and the exact scale, as tests/test_linkmrc_gpu.py's: 5.8e-6 at R = 8.  Both are below
TAU_CAP = 1e-5.  The loss is compared as tests/test_linksoft_gpu.py compares it (``derived_e_s``): the softplus terms are the soft
kernel's, a thread adds the 2 m terms of one pair per pass, and on these grids the (line, slot) walk makes as many passes over its
256 threads as the pair walk ``derived_e_s`` counts (4 on the default grid, 1 on the others).

Measured on one MI355X (the figures this file prints): see DESIGN.md, "Transmit diversity on the link"."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkAlamoutiPlan, LinkMrcPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, PAIRINGS, BlockErrorAccumulator, CodeConfig,
                                      LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig, alamouti_pairs, alamouti_weights,
                                      link_alamouti_host, link_decode_host, link_ldpc_host, noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linkalamouti import AL_GRIDS, LARGE, STRADDLE, al_cases, al_inputs
from test_linkmrc import MRC_ODD
from test_linksim import SHARE_CAP, TAU_CAP, flagged_share
from test_linksim_gpu import U, _dev
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7777
FACTORS = np.asarray(DEFAULT_FACTORS[:3], dtype=np.float32)
PAIR_IDS = {"time": _abi.AFT_LINK_PAIR_TIME, "frequency": _abi.AFT_LINK_PAIR_FREQUENCY}


def _e_c_and_e_p(R: int):
    e_x = (1 + U) ** 2 - 1
    e_h = (1 + e_x) * (1 + U) ** 2 - 1
    e_r = (1 + 3 * U) * (1 + 6 * U) * (1 + U) - 1
    e_n = e_r + np.sqrt(2.0) * 8 * U * (1 + e_r)
    e_y = (1 + max(e_h, e_n)) * (1 + U) ** 3 - 1
    e_c1 = e_y + 2 * U * (1 + e_y)
    return float((1 + e_c1) * (1 + U) ** (2 * R) - 1), float((1 + U) ** (2 + 2 * R) - 1)


def derived_tau(R: int) -> float:
    e_c, e_p = _e_c_and_e_p(R)
    return max(e_c, float((1 + e_p) * (1 + U) ** 3 - 1))


def derived_e_lambda(R: int) -> float:
    e_c, e_p = _e_c_and_e_p(R)
    e_a = (1 + U) ** 2 - 1
    e_i = max((1 + e_a) * (1 + e_p), 1 + e_c) * (1 + U) - 1
    e_mu = (1 + e_a) * (1 + U) * (1 + e_i) - 1
    e_d = 2 * e_mu + 2 * U * (1 + e_mu)
    return float(e_d + U * (2 + e_d))


def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    for R in (1, 2, 3, 4, 8):
        print(f"R = {R}: tau = {derived_tau(R):.3e} = {derived_tau(R) / U:.1f} u, e_lambda = {derived_e_lambda(R):.3e} = "
              f"{derived_e_lambda(R) / U:.1f} u")
    assert derived_tau(1) < derived_tau(2) < derived_tau(8) and derived_e_lambda(1) < derived_e_lambda(8)
    assert derived_tau(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


_plans, _ops, _wants = {}, {}, {}


def _plan(name, m, R, pairing):
    if (name, m, R, pairing) not in _plans:
        _plans[name, m, R, pairing] = LinkAlamoutiPlan(LinkConfig(al_inputs(name)[0], m), DEV, R, pairing)
    return _plans[name, m, R, pairing]


def _operands(name, R, which="lmmse"):
    """The frames whole groups of 2 R fill, on the host and on the device: (n, (ideal, est, keys, sigma, rho, scale)) twice, in the
    order the plan takes them."""
    if (name, R, which) not in _ops:
        sim, keys, sigma, snr, ideal, est = al_inputs(name)
        n = len(keys) // (2 * R) * 2 * R
        host = (ideal[:n], est[which][:n], keys[:n], sigma[:n], *alamouti_weights(snr[:n], 0.0, R))
        _ops[name, R, which] = (n, host, tuple(_dev(a) for a in host))
    return _ops[name, R, which]


def _run(name, m, R, pairing, which="lmmse", want_llr=True, lib=None):
    return _plan(name, m, R, pairing)(*_operands(name, R, which)[2], _dev(FACTORS), want_llr=want_llr, lib=lib)


def _want(name, m, R, pairing, which):
    """The definition at tau(R) and e_lambda(R), computed once: (counts, loss, llr, wrong, flags, loss_lo, loss_hi, q)."""
    if (name, m, R, pairing, which) not in _wants:
        _, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R, which)
        _wants[name, m, R, pairing, which] = link_alamouti_host(LinkConfig(al_inputs(name)[0], m), keys, ideal, est, sigma, rho, scale, R,
                                                                pairing, FACTORS, tau=derived_tau(R), e_lambda=derived_e_lambda(R))
    return _wants[name, m, R, pairing, which]


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m, pairing):
    rows = with_flags = differing = 0
    worst_llr = worst_share = worst_loss = 0.0
    for name, R, n in al_cases():
        cfg = LinkConfig(al_inputs(name)[0], m)
        e_s, e_l = derived_e_s(cfg), derived_e_lambda(R)
        for which in ("lmmse", "ideal"):
            want_counts, _, want_llr, _, flags, lo, hi, q = _want(name, m, R, pairing, which)
            counts, loss, llr = _run(name, m, R, pairing, which)
            G = n // (2 * R)
            assert counts.shape == (G, 2) and counts.dtype == torch.int32 and loss.shape == (G, 3) and llr.shape == (G, *cfg.sim.ofdm, m)
            if name in LARGE:
                share = flagged_share(cfg, flags)
                assert share <= SHARE_CAP, (name, R, which, share)
                worst_share = max(worst_share, share)
            else:
                assert flags.sum() <= 1, (name, R, which, int(flags.sum()))
            got = counts.cpu().numpy().astype(np.int64)
            pairs, elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
            assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= pairs).all(), (name, R, which, got, want_counts, pairs)
            assert (np.abs(got[:, 1] - want_counts[:, 1]) <= elems).all(), (name, R, which, got, want_counts, elems)
            got_llr = llr.cpu().numpy().astype(np.float64)
            err = np.abs(got_llr - want_llr)
            ratio = float((err[q > 0] / q[q > 0] / e_l).max())
            print(f"  {name} R = {R} {pairing} {which}: |llr_dev - llr_def| / (e_lambda q) = {ratio:.3f}")
            assert np.isfinite(got_llr).all() and (err <= e_l * q).all(), (name, R, which, ratio)
            got_loss = loss.cpu().numpy().astype(np.float64)
            assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                (name, R, which, got_loss, lo, hi)
            width = np.maximum(hi * (1 + e_s) - lo * (1 - e_s), FLOOR)
            worst_loss = max(worst_loss, float((np.abs(got_loss - (lo + hi) / 2) / (width / 2)).max()))
            rows += G
            with_flags += int((pairs > 0).sum())
            differing += int((got != want_counts).any(axis=1).sum())
            worst_llr = max(worst_llr, ratio)
    print(f"m = {m}, {pairing}: {with_flags} of {rows} groups had a flagged decision at tau(R); {differing} differ from the definition; "
          f"largest flagged share {worst_share:.2e}; largest |llr_dev - llr_def| / (e_lambda(R) q) = {worst_llr:.2f}; the loss sits "
          f"within {worst_loss:.2f} of its interval's half-width from the middle")


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_antenna_is_the_diversity_kernel_bit_for_bit(m, pairing):
    """With ``H_r1 = E_r1 = 0`` the sample is ``link_branch``'s and the second term of every sum an exact zero: the LLRs at first and
    lone elements are ``LinkMrcPlan``'s on the frames (r, 0)."""
    f = _dev(FACTORS)
    for name, R, _ in al_cases():
        cfg = LinkConfig(al_inputs(name)[0], m)
        _, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        _, _, llr = _plan(name, m, R, pairing)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale)), f, want_llr=True)
        mrc = tuple(_dev(np.ascontiguousarray(a)) for a in (ideal[::2], est[::2], keys[::2], sigma[::2], rho[::2], scale))
        _, _, want = LinkMrcPlan(cfg, DEV, R)(*mrc, f, want_llr=True)
        role = alamouti_pairs(cfg, pairing)[0]
        heard = torch.from_numpy((role == 0) | (role == 2)).to(DEV)
        assert heard.any() and torch.equal(llr[:, heard], want[:, heard]), (name, R)
        assert llr.isfinite().all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    f = _dev(FACTORS)
    for name in LARGE:
        sim, keys, sigma, snr, ideal, est = al_inputs(name)
        for R, pairing in ((1, "time"), (2, "frequency"), (3, "time")):
            p, W = _plan(name, m, R, pairing), 2 * R
            idx = (np.arange(37 * W) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-W:] = np.arange(W, 2 * W)                                       # ... the last one group 1 of ``_operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est["lmmse"][i]), _dev(keys[i]), _dev(sigma[i]),  # noqa: E731
                             *(_dev(a) for a in alamouti_weights(snr[i], 0.0, R)))
            batch = p(*ops(idx), f, want_llr=True)
            alone = p(*ops(np.arange(W, 2 * W)), f, want_llr=True)
            _same_bits([t[36:37] for t in batch], alone)
            _same_bits([t[1:2] for t in _run(name, m, R, pairing)], alone)       # second of the groups of ``_operands``
            _same_bits(p(*ops(idx), f, want_llr=True), batch)                    # a second run of the same batch


def _entry(plan, ops, factors, counts, loss, llr, batch, hp=None, ep=None, lib=None):
    h, e, *rest = ops
    return (lib or _lib.load()).aft_link_alamouti_f32(
        ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), *(t.data_ptr() for t in rest), factors.data_ptr(), factors.numel(),
        *plan.group, counts.data_ptr(), loss.data_ptr(), llr, batch, _lib.current_stream_ptr(counts.device))


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m, pairing):
    """Every element of the three outputs is written -- zeros at the pilots included -- and nothing beside them; without the LLR
    output, and with ideal, est and llr 8, 4 and 12 bytes off a 16-byte boundary, the same bits."""
    f = _dev(FACTORS)
    for name, R in (("default_120x14", 2), ("odd_30x7", 3), (STRADDLE, 2)):
        n, _, ops = _operands(name, R)
        p, G = _plan(name, m, R, pairing), n // (2 * R)
        want = _run(name, m, R, pairing)
        mask = torch.from_numpy(p.cfg.data_mask).to(DEV)
        assert (want[2][:, ~mask] == 0).all() and (want[2][:, mask] != 0).any(dim=-1).all()
        h, e = ops[0], ops[1]
        fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
        fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
        assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
        for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (None, fe.data_ptr() + 8, 0), (None, None, 8),
                            (None, None, 4), (fh.data_ptr() + 8, None, 12), (None, None, None)):
            counts = torch.full((G + 1, 2), POISON, dtype=torch.int32, device=DEV)
            loss = torch.full((G + 1, 3), float("nan"), device=DEV)
            llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
            _lib.check(_entry(p, ops, f, counts, loss, None if off is None else llr.data_ptr() + off, n, hp, ep))
            _same_bits([counts[:G], loss[:G]], want[:2])
            assert (counts[G:] == POISON).all() and loss[G:].isnan().all()
            if off is None:
                assert llr.isnan().all()
            else:
                at = off // 4
                _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
        _same_bits(_run(name, m, R, pairing, want_llr=False)[:2], want[:2])
    # 3 x 5: the pilot at (1, 2) carries 0 and the last element (2, 4), lone in both pairings, is written, finite and not a pilot's zero
    n, _, ops = _operands(MRC_ODD, 2)
    counts = torch.full((1, 2), POISON, dtype=torch.int32, device=DEV)
    loss, llr = torch.full((1, 3), float("nan"), device=DEV), torch.full((1, 3, 5, m), float("nan"), device=DEV)
    _lib.check(_entry(_plan(MRC_ODD, m, 2, pairing), ops, f, counts, loss, llr.data_ptr(), n))
    _same_bits([counts, loss, llr], _run(MRC_ODD, m, 2, pairing))
    assert alamouti_pairs(LinkConfig(al_inputs(MRC_ODD)[0], m), pairing)[0][2, 4] == 2
    assert llr.isfinite().all() and (llr[:, 2, 4] != 0).all() and (llr[:, 1, 2] == 0).all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_alamouti_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_alamouti_f32")
    for name, n in AL_GRIDS.items():
        for m in BITS_PER_SYMBOL:
            for R, pairing in ((1, "frequency"), (2, "time"), (2, "frequency"), (8, "time")):
                if n >= 2 * R:
                    _same_bits(_run(name, m, R, pairing, lib=lib), _run(name, m, R, pairing))


def test_what_the_plan_refuses():
    """The batch, then every operand after ``sigma`` too short, then the last of them with another dtype and in pageable host memory,
    then the factors: in the order the plan checks them; then what the constructor refuses."""
    n, _, (h, e, k, s, rho, scale) = _operands("odd_30x7", 4)
    p, f = _plan("odd_30x7", 4, 4, "time"), _dev(FACTORS)
    for args, word in (((h[:6], e[:6], k[:6], s[:6], rho[:6], scale, f), "6 frames is not a multiple of branches \\* 2 = 4 \\* 2"),
                       ((h, e, k, s, rho[:8], scale, f), "rho must hold"), ((h, e, k, s, rho, scale[:3], f), "scale must hold"),
                       ((h, e, k, s, rho, scale.double(), f), "scale must be torch.float32"),
                       ((h, e, k, s, rho, torch.from_numpy(np.zeros(4, np.float32)), f), "pinned host memory"),
                       ((h, e, k, s, rho, scale, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            p(*args)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkAlamoutiPlan(p.cfg, DEV, bad)
    for bad in ("space", 0, None, True):
        with pytest.raises(ValueError, match="pairing"):
            LinkAlamoutiPlan(p.cfg, DEV, 2, bad)
    with pytest.raises(ValueError, match="LinkAlamoutiPlan runs on a HIP device"):
        LinkAlamoutiPlan(p.cfg, "cpu", 2)
    assert LinkAlamoutiPlan(p.cfg, DEV, 1).group == (1, 0) and LinkAlamoutiPlan(p.cfg, DEV, 8, "frequency").group == (8, 1)


def test_every_refusal_of_the_entry_point_launches_nothing():
    name, m, R, pairing = "default_120x14", 4, 2, "frequency"
    n, _, (h, e, k, s, rho, scale) = _operands(name, R)
    lib, G, f = _lib.load(), n // (2 * R), _dev(FACTORS)
    fn = lib.aft_link_alamouti_f32
    cfg = LinkConfig(al_inputs(name)[0], m)
    counts = torch.full((G, 2), POISON, dtype=torch.int32, device=DEV)
    loss = torch.full((G, 3), float("nan"), device=DEV)
    llr = torch.full((G, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), rho=rho.data_ptr(), scale=scale.data_ptr(),
                factors=f.data_ptr(), n_factors=3, branches=R, pairing=PAIR_IDS[pairing], counts=counts.data_ptr(), loss=loss.data_ptr(),
                llr=llr.data_ptr(), batch=n)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return fn(ctypes.byref(p), *(a[x] for x in good), None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert fn(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
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
    for bad in (0, 9, -2):
        refused(SH, f"branches = {bad} is outside 1..8", branches=bad)
    for bad in (2, -1, 7):
        refused(SH, f"pairing = {bad} is neither", pairing=bad)
    refused(E, "batch = 16 is not a multiple of branches * 2 = 3 * 2", branches=3)
    refused(E, "batch = 14 is not a multiple of branches * 2 = 2 * 2", batch=14)
    refused(SH, "branches = 9", branches=9, pairing=5, batch=14)                     # the order: branches, pairing, the group
    refused(SH, "pairing = 5", pairing=5, batch=14)
    torch.cuda.synchronize()
    assert (counts == POISON).all() and loss.isnan().all() and llr.isnan().all()     # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    _same_bits([counts, loss, llr], _run(name, m, R, pairing))                       # ... and the good call writes it all
    # a grid whose only element is a pilot is legal: counts 0, loss 0, LLR 0
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    for pid in PAIR_IDS.values():
        counts.fill_(POISON)
        loss.fill_(float("nan"))
        llr.fill_(float("nan"))
        assert call(one, batch=8, pairing=pid) == _abi.AFT_OK
        torch.cuda.synchronize()
        assert counts[:2].tolist() == [[0, 0]] * 2 and loss[:2].tolist() == [[0.0] * 3] * 2 and llr.reshape(-1)[:2 * m].tolist() == [0.0] * (2 * m)
        assert (counts[2:] == POISON).all() and llr.reshape(-1)[2 * m:].isnan().all()


@pytest.mark.parametrize("kind", ("viterbi", "ldpc"))
def test_coded_accumulators_with_transmit_diversity_run_without_a_synchronisation(kind):
    """``tx_diversity="time"`` at 2 x 2, fed by the simulator's correlated groups of ``antennas=(2, 2)``: the batches run without a
    synchronisation, the errors are the host decoders' on the device's own LLRs with the leaders' keys, frame numbers hashed on the
    device give the same result, and perfect channel knowledge is no worse than the estimate."""
    R, seed, pairing = 2, 2, "time"
    sim = ChannelSimConfig(antennas=(2, 2))
    link = LinkConfig(sim, 4)
    code = CodeConfig(link, 256, "3/4") if kind == "viterbi" else LdpcConfig(link, "1/2")
    make = BlockErrorAccumulator if kind == "viterbi" else LdpcBlockErrorAccumulator
    decode = link_decode_host if kind == "viterbi" else link_ldpc_host
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    with_est, perfect, on_device = (make(code, DEV, seed=seed, branches=R, tx_diversity=pairing) for _ in range(3))
    assert type(with_est._plan) is LinkAlamoutiPlan
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
    groups = 48 // (2 * R)
    assert len(seen) == 3 and with_est.frames == perfect.frames == groups and with_est.errors.is_cuda and with_est.errors.dtype == torch.int64
    p, one = LinkAlamoutiPlan(link, DEV, R, pairing), torch.ones(1, device=DEV)
    want = np.zeros((2, len(with_est.errors)), np.int64)
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        lead = np.ascontiguousarray(keys[::2 * R])
        w = tuple(_dev(a) for a in alamouti_weights(snr, 0.0, R))
        for i, e in enumerate((est, ideal)):
            _, _, llr = p(ideal, e, _dev(keys), _dev(noise_sigma(snr)), *w, one, want_llr=True)
            want[i] += decode(code, lead, llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()     # keys hashed on the device are the host's
    assert with_est.result() == want[0][1] / (groups * code.blocks) and perfect.result() <= with_est.result()
    print(f"{kind}, 2 x 2 Alamouti over {pairing}: BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}")
