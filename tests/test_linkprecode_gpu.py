"""``aft_link_precoded_f32``, ``hip_ops.LinkPrecodedPlan`` and the ``precoding_subband=`` argument of the accumulators on the HIP device:
the kernel's PMIs against the float64 selection (``linksim.precoding_pmi_host``) outside PMI-flagged subbands, and its counts, LLRs
and losses against the float64 definition EVALUATED WITH THE DEVICE'S PMIs (``linksim.link_precoded_host(..., pmi=)``) through the
bounds derived below; an unheard second antenna against the diversity kernel bit for bit, a turn of the second antenna by ``j``,
independence of the batch, of the position and of the run, no unwritten element, bases off 16 bytes, the checked build, the refusals,
and the four accumulators without a synchronisation, the coded ones against the host decoders on the device's own LLRs.

The shapes are tests/test_linkalamouti.py's ``al_inputs`` (seed 3): frames 0..15 of the default grid (1680 elements: seven passes of
the element walk over 256 threads, and with B = S seven elements per thread of the one team that sums the band), 0..31 of 30 x 7 (a
ragged only pass), the four frames of 3 x 5 and 0..15 of 9 x 6, each frame at the SNR it was drawn with, so the weights are mixed; R in
(1, 2, 3, 4, 8) on the frames whole groups of 2 R fill; B in (1, 4, 7, S) where it fits -- one PMI per subcarrier, short last subbands
of 1 of 9 and 2 of 30 subcarriers, one wideband PMI --; the LMMSE estimate and the channel itself.  The selection's teams come in
every width the kernel has on these shapes: 8 threads (3 x 5, 9 x 6 and 30 x 7 at B = 1), 16 (the default grid at B = 1; 3 x 5 at
B = 3), 32, 64 (teams inside a wave; the default grid at B = 7 with two elements per thread), 128 (the default grid at B = 60, the
one width beyond the issue's: two subbands, two waves each) and 256 (the bands of 30 x 7 and of the default grid: four waves), with
rounds that leave teams without a subband.

The selection.  u = 2^-24; every float32 operation errs by at most u times its result; ``rho`` and the estimates are the same float32
numbers on both sides.  A team of W threads sums a subband of n_b = S_b T elements, W = the power of two at or above B T in 8 .. 64,
doubled up to 256 while there are more teams than subbands and fewer threads than elements (``team_width``, the launcher's rule):
thread l adds its elements l, l + W, ... and within an element the antennas in increasing r,
so a thread's chain is k = ceil(n_b / W) R fused multiply-adds, followed by the log2(min(W, 64)) additions of the shuffles and, where
the team is 2 or 4 waves, the 1 or 3 additions of the waves' sums: at most log2(W) + 1.  A term's component is a product and a fused
multiply-add (two roundings, at most 2 u |E_r0||E_r1| each way), and every partial sum is within the sum of the absolute terms, so a
component of the device's g_b is within ((1 + 2 u)(1 + u)^(k + 9) - 1) Gr_b <= (k + 12) u Gr_b of the exact sum, Gr_b = sum rho_r
|E_r0||E_r1|.  The difference of two of v's entries moves by twice that, so tau_pmi(n_b, R) = 2 (ceil(n_b / W) R + 12) u: 8.1e-6 at
the default grid's wideband sum with R = 8 (seven elements per thread), below PMI_TAU_CAP = 1e-4.  The float64 twin's own error (about
n_b R 2^-53) is far inside the slack of 1 u.

The elements follow tests/test_linkalamouti_gpu.py's chain (complex quantities carry a bound on the MAGNITUDE of their error):

* x, H x and the noise as there: e_x, e_h, e_n.  q H_r1 is exact.
* the sample is ``link_sample2``'s on (H_r0, q H_r1) with x twice: e_y = (1 + max(e_h, e_n))(1 + u)^3 - 1 of reach(y_r) = |H_r0||x| +
  |H_r1||x| + |noise|.
* e_r = E_r0 + q E_r1 adds ONE rounding per component to exact inputs: e_e = u of |e_r| <= reach(e_r) = |E_r0| + |E_r1|.
* a term y conj(e) is a product and a fused multiply-add per component on two inexact factors:
  e_c1 = (1 + e_y)(1 + e_e)(1 + 2 u) - 1 of reach(y_r) reach(e_r).
* c takes one term per antenna by one fused multiply-add: e_c(R) = (1 + e_c1)(1 + u)^R - 1 of reach(c).
* |e|^2 is rounded twice on a factor within e_e, then R fused multiply-adds: e_p(R) = (1 + e_e)^2 (1 + u)^(2 + R) - 1 of p_reach =
  sum rho reach(e_r)^2 >= p -- e_r cancels, so p's error is not relative to p itself --; the threshold beta_b p adds the three roundings
  of tests/test_linksim_gpu.py.

tau(R) = max(e_c(R), (1 + e_p(R))(1 + u)^3 - 1): 2.1e-6 at R = 8.  e_lambda(R) is tests/test_linksoft_gpu.py's chain with e_c(R) and
e_p(R) in place of its e_c and e_p and the exact scale: 4.9e-6 at R = 8.  Both are below TAU_CAP = 1e-5.  The loss is compared as
tests/test_linksoft_gpu.py compares it (``derived_e_s``): the softplus terms are the soft kernel's; a thread of the element walk adds
the m terms of ceil(S T / 256) elements, never more than the 2 m terms of ceil(ceil(S T / 2) / 256) pairs ``derived_e_s`` counts.

Measured on one MI355X (the figures this file prints): see DESIGN.md, "Closed-loop precoding on the link"."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkMrcPlan, LinkPrecodedPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator,
                                      LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator, link_decode_host, link_ldpc_host,
                                      link_precoded_host, noise_sigma, precoding_pmi_host, precoding_weights)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linkalamouti import AL_GRIDS, LARGE, STRADDLE, al_cases, al_inputs
from test_linkmrc import MRC_ODD
from test_linkprecode import PMI_TAU_CAP, ROTATED, SUBBANDS, pc_cases, widths
from test_linksim import SHARE_CAP, TAU_CAP, flagged_share
from test_linksim_gpu import U, _dev
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7777
FACTORS = np.asarray(DEFAULT_FACTORS[:3], dtype=np.float32)


def team_width(elements: int, n_sub: int) -> int:
    """The threads that sum a subband where a whole one holds ``elements`` elements and there are ``n_sub``: the launcher's rule."""
    w = 8
    while w < 64 and w < elements:
        w *= 2
    while w < 256 and 256 // w > n_sub and w < elements:
        w *= 2
    return w


def derived_tau_pmi(elements: int, R: int, n_sub: int) -> float:
    """The margin of the selection where a whole subband holds ``elements`` elements; module docstring."""
    return float(2 * (-(-elements // team_width(elements, n_sub)) * R + 12) * U)


def _tau_pmi(name, R, B) -> float:
    S, T = al_inputs(name)[0].ofdm
    return derived_tau_pmi(min(B, S) * T, R, -(-S // B))


def _e_c_and_e_p(R: int):
    e_x = (1 + U) ** 2 - 1
    e_h = (1 + e_x) * (1 + U) ** 2 - 1
    e_r = (1 + 3 * U) * (1 + 6 * U) * (1 + U) - 1
    e_n = e_r + np.sqrt(2.0) * 8 * U * (1 + e_r)
    e_y = (1 + max(e_h, e_n)) * (1 + U) ** 3 - 1
    e_e = U
    e_c1 = (1 + e_y) * (1 + e_e) * (1 + 2 * U) - 1
    return float((1 + e_c1) * (1 + U) ** R - 1), float((1 + e_e) ** 2 * (1 + U) ** (2 + R) - 1)


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


def test_the_derived_bounds_are_below_the_caps():
    for R in (1, 2, 3, 4, 8):
        print(f"R = {R}: tau = {derived_tau(R):.3e} = {derived_tau(R) / U:.1f} u, e_lambda = {derived_e_lambda(R):.3e} = "
              f"{derived_e_lambda(R) / U:.1f} u, tau_pmi of the default grid's band = {derived_tau_pmi(120 * 14, R, 1):.3e}")
    assert derived_tau(1) < derived_tau(2) < derived_tau(8) and derived_e_lambda(1) < derived_e_lambda(8)
    assert derived_tau(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP
    worst = max(_tau_pmi(name, R, B) for name, R, _, B in pc_cases())
    assert worst == derived_tau_pmi(120 * 14, 8, 1) and worst <= PMI_TAU_CAP
    S_T = {name: al_inputs(name)[0].ofdm for name in AL_GRIDS}
    assert {team_width(B * S_T[name][1], -(-S_T[name][0] // B)) for name, _, _, B in pc_cases()} == {8, 16, 32, 64, 128, 256}
    assert team_width(60 * 14, 2) == 128 and team_width(12 * 14, 10) == 64 and team_width(7 * 14, 18) == 64


_plans, _ops = {}, {}


def _plan(name, m, R, B):
    if (name, m, R, B) not in _plans:
        _plans[name, m, R, B] = LinkPrecodedPlan(LinkConfig(al_inputs(name)[0], m), DEV, R, B)
    return _plans[name, m, R, B]


def _operands(name, R, which="lmmse"):
    """The frames whole groups of 2 R fill, on the host and on the device: (n, (ideal, est, keys, sigma, rho, scale)) twice, in the
    order the plan takes them."""
    if (name, R, which) not in _ops:
        sim, keys, sigma, snr, ideal, est = al_inputs(name)
        n = len(keys) // (2 * R) * 2 * R
        host = (ideal[:n], est[which][:n], keys[:n], sigma[:n], *precoding_weights(snr[:n], 0.0, R))
        _ops[name, R, which] = (n, host, tuple(_dev(a) for a in host))
    return _ops[name, R, which]


def _run(name, m, R, B, which="lmmse", want_llr=True, lib=None):
    return _plan(name, m, R, B)(*_operands(name, R, which)[2], _dev(FACTORS), want_llr=want_llr, lib=lib)


@pytest.mark.parametrize("band", SUBBANDS)
@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m, band):
    rows = with_flags = differing = subbands = pmi_flagged = pmi_differing = 0
    worst_llr = worst_share = worst_loss = 0.0
    for name, R, n in al_cases():
        cfg = LinkConfig(al_inputs(name)[0], m)
        B = cfg.sim.ofdm[0] if band is None else band
        if band is not None and band >= cfg.sim.ofdm[0]:
            continue                                                             # the band itself is the case band = None
        e_s, e_l, tau_pmi = derived_e_s(cfg), derived_e_lambda(R), _tau_pmi(name, R, B)
        for which in ("lmmse", "ideal"):
            _, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R, which)
            counts, loss, llr, pmi = _run(name, m, R, B, which)
            G, n_sub = n // (2 * R), -(-cfg.sim.ofdm[0] // B)
            assert counts.shape == (G, 2) and counts.dtype == torch.int32 and loss.shape == (G, 3) and llr.shape == (G, *cfg.sim.ofdm, m)
            assert pmi.shape == (G, n_sub) and pmi.dtype == torch.int32
            got_pmi = pmi.cpu().numpy()
            want_pmi, pflags = precoding_pmi_host(cfg, est, rho, R, B, tau_pmi)
            assert got_pmi.min() >= 0 and got_pmi.max() <= 3 and pflags.sum() <= 1, (name, R, B, which)
            assert np.array_equal(got_pmi[~pflags], want_pmi[~pflags]), (name, R, B, which)
            subbands += pflags.size
            pmi_flagged += int(pflags.sum())
            pmi_differing += int((got_pmi != want_pmi).sum())
            # everything downstream of the selection: the definition evaluated with the device's PMIs
            want_counts, _, want_llr, _, flags, lo, hi, q, _ = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, FACTORS,
                                                                                 tau=derived_tau(R), e_lambda=e_l, pmi=got_pmi)
            if name in LARGE:
                share = flagged_share(cfg, flags)
                assert share <= SHARE_CAP, (name, R, B, which, share)
                worst_share = max(worst_share, share)
            else:
                assert flags.sum() <= 1, (name, R, B, which, int(flags.sum()))
            got = counts.cpu().numpy().astype(np.int64)
            pairs, elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
            assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= pairs).all(), (name, R, B, which, got, want_counts, pairs)
            assert (np.abs(got[:, 1] - want_counts[:, 1]) <= elems).all(), (name, R, B, which, got, want_counts, elems)
            got_llr = llr.cpu().numpy().astype(np.float64)
            err = np.abs(got_llr - want_llr)
            ratio = float((err[q > 0] / q[q > 0] / e_l).max())
            print(f"  {name} R = {R} B = {B} {which}: |llr_dev - llr_def| / (e_lambda q) = {ratio:.3f}")
            assert np.isfinite(got_llr).all() and (err <= e_l * q).all(), (name, R, B, which, ratio)
            got_loss = loss.cpu().numpy().astype(np.float64)
            assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all(), \
                (name, R, B, which, got_loss, lo, hi)
            width = np.maximum(hi * (1 + e_s) - lo * (1 - e_s), FLOOR)
            worst_loss = max(worst_loss, float((np.abs(got_loss - (lo + hi) / 2) / (width / 2)).max()))
            rows += G
            with_flags += int((pairs > 0).sum())
            differing += int((got != want_counts).any(axis=1).sum())
            worst_llr = max(worst_llr, ratio)
    assert rows > 0
    print(f"m = {m}, B = {'S' if band is None else band}: {pmi_flagged} of {subbands} subbands PMI-flagged at tau_pmi, {pmi_differing} PMIs "
          f"differ from the definition's; {with_flags} of {rows} groups had a flagged decision at tau(R); {differing} differ from the "
          f"definition; largest flagged share {worst_share:.2e}; largest |llr_dev - llr_def| / (e_lambda(R) q) = {worst_llr:.2f}; the "
          f"loss sits within {worst_loss:.2f} of its interval's half-width from the middle")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_second_antenna_is_the_diversity_kernel_bit_for_bit(m):
    """With ``H_r1 = E_r1 = 0`` every subband's sum is 0 and every PMI 0, the sample is ``link_branch``'s and ``e_r = E_r0``: the LLRs
    are ``LinkMrcPlan``'s on the frames (r, 0) at every element."""
    f = _dev(FACTORS)
    for name, R, _, B in pc_cases():
        cfg = LinkConfig(al_inputs(name)[0], m)
        _, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        _, _, llr, pmi = _plan(name, m, R, B)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale)), f, want_llr=True)
        mrc = tuple(_dev(np.ascontiguousarray(a)) for a in (ideal[::2], est[::2], keys[::2], sigma[::2], rho[::2], scale))
        _, _, want = LinkMrcPlan(cfg, DEV, R)(*mrc, f, want_llr=True)
        assert torch.equal(llr, want) and llr.isfinite().all() and not pmi.any(), (name, R, B)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_turn_of_the_second_antenna_by_j(m):
    """``H_r1, E_r1 -> j H_r1, j E_r1``: the subband sums turn exactly, so the PMIs are permuted 0 -> 3, 1 -> 2, 2 -> 0, 3 -> 1 --
    asserted at the twin's unflagged subbands --, q H_r1 and q E_r1 hold the same bits and counts, losses and LLRs are bit-equal."""
    f = _dev(FACTORS)
    for name, R, _, B in pc_cases():
        cfg = LinkConfig(al_inputs(name)[0], m)
        _, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 1j * ideal[1::2], 1j * est[1::2]
        assert np.array_equal(E[1::2].real, -est[1::2].imag) and np.array_equal(E[1::2].imag, est[1::2].real)
        got = _plan(name, m, R, B)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale)), f, want_llr=True)
        want = _run(name, m, R, B)
        clear = ~precoding_pmi_host(cfg, est, rho, R, B, _tau_pmi(name, R, B))[1]
        assert np.array_equal(got[3].cpu().numpy()[clear], ROTATED[want[3].cpu().numpy()][clear]), (name, R, B)
        _same_bits(got[:3], want[:3])


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    f = _dev(FACTORS)
    for name in LARGE:
        sim, keys, sigma, snr, ideal, est = al_inputs(name)
        for R, B in ((1, 1), (2, 7), (3, sim.ofdm[0])):
            p, W = _plan(name, m, R, B), 2 * R
            idx = (np.arange(37 * W) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-W:] = np.arange(W, 2 * W)                                       # ... the last one group 1 of ``_operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est["lmmse"][i]), _dev(keys[i]), _dev(sigma[i]),  # noqa: E731
                             *(_dev(a) for a in precoding_weights(snr[i], 0.0, R)))
            batch = p(*ops(idx), f, want_llr=True)
            alone = p(*ops(np.arange(W, 2 * W)), f, want_llr=True)
            _same_bits([t[36:37] for t in batch], alone)
            _same_bits([t[1:2] for t in _run(name, m, R, B)], alone)             # second of the groups of ``_operands``
            _same_bits(p(*ops(idx), f, want_llr=True), batch)                    # a second run of the same batch


def _entry(plan, ops, factors, counts, loss, llr, pmi, batch, hp=None, ep=None, lib=None):
    h, e, *rest = ops
    return (lib or _lib.load()).aft_link_precoded_f32(
        ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), *(t.data_ptr() for t in rest), factors.data_ptr(), factors.numel(),
        *plan.group, counts.data_ptr(), loss.data_ptr(), llr, pmi.data_ptr(), batch, _lib.current_stream_ptr(counts.device))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m):
    """Every element of the four outputs is written -- zeros at the pilots included -- and nothing beside them; without the LLR
    output, and with ideal, est and llr 8, 4 and 12 bytes off a 16-byte boundary, the same bits."""
    f = _dev(FACTORS)
    for name, R, B in (("default_120x14", 2, 7), ("odd_30x7", 3, 4), (STRADDLE, 2, 9), (MRC_ODD, 2, 1)):
        n, _, ops = _operands(name, R)
        p, G = _plan(name, m, R, B), n // (2 * R)
        want = _run(name, m, R, B)
        mask = torch.from_numpy(p.cfg.data_mask).to(DEV)
        assert (want[2][:, ~mask] == 0).all() and (want[2][:, mask] != 0).any(dim=-1).all() and want[2].isfinite().all()
        h, e = ops[0], ops[1]
        fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
        fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
        assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
        for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (None, fe.data_ptr() + 8, 0), (None, None, 8),
                            (None, None, 4), (fh.data_ptr() + 8, None, 12), (None, None, None)):
            counts = torch.full((G + 1, 2), POISON, dtype=torch.int32, device=DEV)
            loss = torch.full((G + 1, 3), float("nan"), device=DEV)
            llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
            pmi = torch.full((G + 1, p.n_sub), POISON, dtype=torch.int32, device=DEV)
            _lib.check(_entry(p, ops, f, counts, loss, None if off is None else llr.data_ptr() + off, pmi, n, hp, ep))
            _same_bits([counts[:G], loss[:G], pmi[:G]], [want[0], want[1], want[3]])
            assert (counts[G:] == POISON).all() and loss[G:].isnan().all() and (pmi[G:] == POISON).all()
            if off is None:
                assert llr.isnan().all()
            else:
                at = off // 4
                _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
        got = _run(name, m, R, B, want_llr=False)
        assert got[2] is None
        _same_bits([got[0], got[1], got[3]], [want[0], want[1], want[3]])


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_precoded_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_precoded_f32")
    for name, n in AL_GRIDS.items():
        for m in BITS_PER_SYMBOL:
            for R, B in ((1, widths(name)[-1]), (2, 1), (2, widths(name)[1]), (8, 7)):
                if n >= 2 * R and B in widths(name):
                    _same_bits(_run(name, m, R, B, lib=lib), _run(name, m, R, B))


def test_what_the_plan_refuses():
    """The batch, then every operand after ``sigma`` too short, then the last of them with another dtype and in pageable host memory,
    then the factors: in the order the plan checks them; then what the constructor refuses."""
    n, _, (h, e, k, s, rho, scale) = _operands("odd_30x7", 4)
    p, f = _plan("odd_30x7", 4, 4, 7), _dev(FACTORS)
    for args, word in (((h[:6], e[:6], k[:6], s[:6], rho[:6], scale, f), "6 frames is not a multiple of branches \\* 2 = 4 \\* 2"),
                       ((h, e, k, s, rho[:8], scale, f), "rho must hold"), ((h, e, k, s, rho, scale[:3], f), "scale must hold"),
                       ((h, e, k, s, rho, scale.double(), f), "scale must be torch.float32"),
                       ((h, e, k, s, rho, torch.from_numpy(np.zeros(4, np.float32)), f), "pinned host memory"),
                       ((h, e, k, s, rho, scale, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            p(*args)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkPrecodedPlan(p.cfg, DEV, bad, 7)
    for bad in (0, 31, -4, 2.0, None, True, "7"):
        with pytest.raises(ValueError, match="subband"):
            LinkPrecodedPlan(p.cfg, DEV, 2, bad)
    with pytest.raises(ValueError, match="1025 subbands of the 1025 subcarriers, more than 1024"):
        LinkPrecodedPlan(LinkConfig(ChannelSimConfig(ofdm=(1025, 2), pilot=(5, 2)), 2), DEV, 1, 1)
    with pytest.raises(ValueError, match="LinkPrecodedPlan runs on a HIP device"):
        LinkPrecodedPlan(p.cfg, "cpu", 2, 7)
    one, band = LinkPrecodedPlan(p.cfg, DEV, 1, 1), LinkPrecodedPlan(p.cfg, DEV, 8, 30)
    assert (one.group, one.n_sub, band.group, band.n_sub, p.n_sub) == ((1, 1), 30, (8, 30), 1, 5)


def test_every_refusal_of_the_entry_point_launches_nothing():
    """Every refusal of this entry point is AFT_ERR_ARG."""
    name, m, R, B = "default_120x14", 4, 2, 7
    n, _, (h, e, k, s, rho, scale) = _operands(name, R)
    lib, G, f = _lib.load(), n // (2 * R), _dev(FACTORS)
    fn = lib.aft_link_precoded_f32
    cfg = LinkConfig(al_inputs(name)[0], m)
    counts = torch.full((G, 2), POISON, dtype=torch.int32, device=DEV)
    loss = torch.full((G, 3), float("nan"), device=DEV)
    llr = torch.full((G, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    pmi = torch.full((G, 120), POISON, dtype=torch.int32, device=DEV)            # room for B = 1
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), rho=rho.data_ptr(), scale=scale.data_ptr(),
                factors=f.data_ptr(), n_factors=3, branches=R, subband=B, counts=counts.data_ptr(), loss=loss.data_ptr(),
                llr=llr.data_ptr(), pmi=pmi.data_ptr(), batch=n)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return fn(ctypes.byref(p), *(a[x] for x in good), None)

    def refused(word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == _abi.AFT_ERR_ARG and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    assert fn(None, *good.values(), None) == _abi.AFT_ERR_ARG and "NULL pointer" in lib.aft_last_error().decode()
    for x in ("ideal", "est", "keys", "sigma", "rho", "scale", "factors", "counts", "loss", "pmi"):
        refused("NULL pointer", **{x: None})
    for x in ("ideal", "est", "keys"):
        refused("8-byte", **{x: good[x] + 4})
    for x in ("sigma", "rho", "scale", "factors", "counts", "loss", "llr", "pmi"):
        refused("4-byte", **{x: good[x] + 2})
    for batch in (0, -3):
        refused("batch must be at least 1", batch=batch)
    for nf in (0, 9, -1):
        refused(f"n_factors = {nf} is outside 1..8", n_factors=nf)

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
        refused(word, p=struct(**fields))
    for bad in (0, 9, -2):
        refused(f"branches = {bad} is outside 1..8", branches=bad)
    for bad in (0, 121, -1):
        refused(f"subband = {bad} is outside 1..120", subband=bad)
    refused("batch = 16 is not a multiple of branches * 2 = 3 * 2", branches=3)
    refused("batch = 14 is not a multiple of branches * 2 = 2 * 2", batch=14)
    refused("branches = 9", branches=9, subband=0, batch=14)                         # the order: branches, the group, the subbands
    refused("batch = 14", subband=0, batch=14)
    refused("subband = 1 makes 2048 subbands of the 2048 subcarriers, more than 1024", p=struct(num_scs=2048), subband=1)
    torch.cuda.synchronize()
    assert (counts == POISON).all() and loss.isnan().all() and llr.isnan().all() and (pmi == POISON).all()     # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    want = _run(name, m, R, B)
    _same_bits([counts, loss, llr, pmi.reshape(-1)[:G * 18]], [*want[:3], want[3].reshape(-1)])      # ... and the good call writes it all
    assert (pmi.reshape(-1)[G * 18:] == POISON).all()
    # a grid whose only element is a pilot is legal: counts 0, loss 0, LLR 0, and the one subband's sum is the estimates' own
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    counts.fill_(POISON)
    loss.fill_(float("nan"))
    llr.fill_(float("nan"))
    pmi.fill_(POISON)
    assert call(one, batch=8, subband=1) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert counts[:2].tolist() == [[0, 0]] * 2 and loss[:2].tolist() == [[0.0] * 3] * 2 and llr.reshape(-1)[:2 * m].tolist() == [0.0] * (2 * m)
    assert (counts[2:] == POISON).all() and llr.reshape(-1)[2 * m:].isnan().all()
    assert all(0 <= v <= 3 for v in pmi.reshape(-1)[:2].tolist()) and (pmi.reshape(-1)[2:] == POISON).all()


def test_the_four_accumulators_with_precoding_run_without_a_synchronisation():
    """``precoding_subband=12`` at 2 x 2, fed by the simulator's correlated groups of ``antennas=(2, 2)``: the batches run without a
    synchronisation; the errors, losses and the PMI histogram are the plan's own, the coded accumulators' errors the host decoders' on
    the device's own LLRs with the leaders' keys, frame numbers hashed on the device give the same result, and perfect channel
    knowledge is no worse than the estimate."""
    R, seed, B = 2, 2, 12
    sim = ChannelSimConfig(antennas=(2, 2))
    link = LinkConfig(sim, 4)
    conv_code, ldpc_code = CodeConfig(link, 256, "3/4"), LdpcConfig(link, "1/2")
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    kw = dict(seed=seed, branches=R, precoding_subband=B)
    hard, rate = LinkAccumulator(link, DEV, **kw), RateAccumulator(link, DEV, factors=(1.0, 0.5), **kw)
    conv, ldpc = BlockErrorAccumulator(conv_code, DEV, **kw), LdpcBlockErrorAccumulator(ldpc_code, DEV, **kw)
    perfect, on_device = BlockErrorAccumulator(conv_code, DEV, **kw), BlockErrorAccumulator(conv_code, DEV, **kw)
    assert all(type(a._plan) is LinkPrecodedPlan for a in (hard, rate, conv, ldpc))
    it = iter(loader)
    first = next(it)
    seen = []

    def step(batch):
        pil, ideal, meta = batch
        est = model(pil, meta)
        for acc in (hard, rate, conv, ldpc):
            acc.update(est, ideal, meta)
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
    assert len(seen) == 3 and all(a.frames == groups for a in (hard, rate, conv, ldpc, perfect))
    assert hard.errors.is_cuda and hard.errors.dtype == torch.int64 and hard._pmi_counts.is_cuda
    p, one, two = LinkPrecodedPlan(link, DEV, R, B), torch.ones(1, device=DEV), _dev(np.asarray([1.0, 0.5], np.float32))
    want = {"hard": np.zeros(2, np.int64), "loss": torch.zeros(2, dtype=torch.float64, device=DEV), "pmi": np.zeros(4, np.int64),
            "conv": np.zeros(2, np.int64), "ldpc": np.zeros(3, np.int64), "perfect": np.zeros(2, np.int64)}
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        lead = np.ascontiguousarray(keys[::2 * R])
        w = tuple(_dev(a) for a in precoding_weights(snr, 0.0, R))
        counts, loss, _, pmi = p(ideal, est, _dev(keys), _dev(noise_sigma(snr)), *w, two)
        want["hard"] += counts.cpu().numpy().sum(axis=0)
        want["loss"] += loss.sum(dim=0, dtype=torch.float64)
        want["pmi"] += np.bincount(pmi.cpu().numpy().reshape(-1), minlength=4)
        _, _, llr, _ = p(ideal, est, _dev(keys), _dev(noise_sigma(snr)), *w, one, want_llr=True)
        want["conv"] += link_decode_host(conv_code, lead, llr.cpu().numpy())[0].sum(axis=0)
        want["ldpc"] += link_ldpc_host(ldpc_code, lead, llr.cpu().numpy())[0].sum(axis=0)
        _, _, llr, _ = p(ideal, ideal, _dev(keys), _dev(noise_sigma(snr)), *w, one, want_llr=True)
        want["perfect"] += link_decode_host(conv_code, lead, llr.cpu().numpy())[0].sum(axis=0)
    assert hard.errors.cpu().tolist() == want["hard"].tolist() and torch.equal(rate.loss, want["loss"])
    assert conv.errors.cpu().tolist() == want["conv"].tolist() and ldpc.errors.cpu().tolist() == want["ldpc"].tolist()
    assert perfect.errors.cpu().tolist() == want["perfect"].tolist()
    assert on_device.errors.cpu().tolist() == conv.errors.cpu().tolist()             # keys hashed on the device are the host's
    for acc in (hard, rate, conv, ldpc, on_device):
        assert acc.pmi_histogram() == want["pmi"].tolist() and sum(acc.pmi_histogram()) == groups * 10
    assert conv.result() == want["conv"][1] / (groups * conv_code.blocks) and perfect.result() <= conv.result()
    print(f"2 x 2 precoded, B = {B}: BER {hard.result():.4f}, GMI {rate.result_gmi():.3f}; Viterbi BLER with the LMMSE estimate "
          f"{conv.result():.3f}, with the channel {perfect.result():.3f}; LDPC BLER {ldpc.result():.3f}; PMI histogram {hard.pmi_histogram()}")
