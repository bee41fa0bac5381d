"""``aft_link_cancel_f32`` (``hip_ops.LinkCancelPlan``), ``aft_link_ldpc_masked_f32`` (``hip_ops.LinkLdpcPlan(..., mask=)``) and
``detector="cwsic"`` on the HIP device.

The cancel kernel against the float64 twin (``linksim.link_cancel_host``) over tests/test_linksm.py's ``sm_cases`` with the LMMSE
estimate and the channel itself at every modulation order.  ``failed`` cycles the four (f0, f1) patterns over the groups, starting at
pattern k when it is read at stride k (k = 1, 2, 3), so a case with one group still sees three patterns; ``state`` is the truth table
exactly and a stream without ``redo`` is exactly zero.  A re-detected stream is compared through the bounds tests/test_linksic_gpu.py
derives for the successive-cancellation kernel's second stage -- the same ``link_sic_cancel`` chain; the cancelled symbol is the sent
one, formed by the same expression on both sides, so its ``e_x`` is already inside ``e_c2`` --: ``derived_tau_sic(R)`` for the flags
(a flagged (element, axis) may move the bit count by one, an element with a flag the symbol count by one), ``derived_e_lambda_sic(R)``
for the LLRs in units of q, ``derived_e_s`` for the losses against the twin's interval.  The twin's flagged share stays below
``SM_SHARE_CAP`` on these inputs, checked on the CPU side of the test.

Two identities hold bit for bit: with an unheard stream 1 a re-detected stream 0 is ``aft_link_mrc_f32`` on the frames (r, 0); and
wherever ``aft_link_sic_f32`` detected a stream second after a correct first decision (outside the definition's dependent set, where
the device's order and first decision are the definition's), its second-stage LLRs are this kernel's.

The masked decoder is integer after the quantiser: selected frames equal ``link_ldpc_host`` and ``aft_link_ldpc_f32`` exactly, the
others are zeros.  The chain of four launches is exact stage by stage against the host definitions fed the device's own float32 LLRs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import link2_gpu
import test_linkldpc_gpu as ldpc_gpu
from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkCancelPlan, LinkLdpcPlan, LinkMrcPlan, LinkSicPlan, LinkSmPlan, fill_lds
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig, cwsic_final, cwsic_redetect,
                                      link_cancel_host, link_ldpc_host, link_sic_host, noise_sigma, sm_weights)
from adafortitran_amd.lmmse import LmmseEstimator
from link2_gpu import DEV, FACTORS, POISON
from test_chansim_gpu import _no_sync, _same_bits
from test_linkcode import SIMS
from test_linkcode_gpu import FRAMES, KEYS
from test_linkcwsic import PATTERNS, PHYSICAL, _all, physical_conditions, physical_inputs
from test_linkmrc import MRC_ODD
from test_linksic import _order, derived_e_lambda_sic, derived_tau_sic
from test_linksim import TAU_CAP
from test_linksim_gpu import _dev, _pinned
from test_linksm import SM_SHARE_CAP, sm_cases, sm_inputs
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
DEFAULT = ChannelSimConfig()
_plans, _twins = {}, {}


def _operands(name, R, which="lmmse"):
    """(n, host operands, device operands) without ``reg``: (ideal, est, keys, sigma, rho, scale)."""
    n, host, dev = link2_gpu.operands("mmse", name, R, which)
    return n, host[:6], dev[:6]


def _plan(name, m, R):
    if (name, m, R) not in _plans:
        _plans[name, m, R] = LinkCancelPlan(LinkConfig(sm_inputs(name)[0], m), DEV, R)
    return _plans[name, m, R]


def _failed(G, shift=0, stride=1):
    """(the pattern int32 [G, 2] -- pattern (g + shift) mod 4 for group g, failed streams with varying non-zero counts --, a device
    view of it with ``stride`` words between the streams' counts)."""
    f = np.asarray([PATTERNS[(g + shift) % 4] for g in range(G)], dtype=np.int32) * (1 + np.arange(G, dtype=np.int32) % 3)[:, None]
    wide = torch.full((2 * G, stride), POISON, dtype=torch.int32, device=DEV)
    wide[:, stride - 1] = _dev(f.reshape(-1))
    return f, wide[:, stride - 1]


def _every(G, s):
    """``failed`` on the device with stream ``s`` of every group failed and the other one acknowledged."""
    f = np.zeros((G, 2), np.int32)
    f[:, s] = 1
    return _dev(f.reshape(-1))


def _run(name, m, R, failed, which="lmmse", want_llr=True, want_state=True, lib=None):
    return _plan(name, m, R)(*_operands(name, R, which)[2], failed, _dev(FACTORS), want_llr=want_llr, want_state=want_state, lib=lib)


def _twin(name, m, R, which):
    """The definition with stream 0 and with stream 1 of every group detected again, at tau_sic(R) and e_lambda_sic(R): computed once."""
    if (name, m, R, which) not in _twins:
        n, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R, which)
        cfg, G = LinkConfig(sm_inputs(name)[0], m), n // (2 * R)
        _twins[name, m, R, which] = [link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, R, _all(G, s), 2, FACTORS,
                                                      tau=derived_tau_sic(R), e_lambda=derived_e_lambda_sic(R)) for s in (0, 1)]
    return _twins[name, m, R, which]


def _entry(plan, ops, failed, stride, factors, counts, loss, llr, state, batch, hp=None, ep=None, lib=None):
    h, e, *rest = ops
    return (lib or _lib.load()).aft_link_cancel_f32(
        ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), *(t.data_ptr() for t in rest), factors.data_ptr(), factors.numel(),
        plan.branches, plan.streams, failed, stride, counts.data_ptr(), loss.data_ptr(), llr, state, batch,
        _lib.current_stream_ptr(counts.device))


# ---- the cancel kernel against the twin ----

def test_the_derived_bounds_are_below_the_cap_at_eight_branches():
    assert derived_tau_sic(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP and derived_e_lambda_sic(_abi.AFT_LINK_MAX_BRANCHES) <= TAU_CAP


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    worst = dict(llr=0.0, bits=0.0, flagged=0.0)
    rows = differing = 0
    for name, R, n in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        e_s, e_l, G = derived_e_s(cfg), derived_e_lambda_sic(R), n // (2 * R)
        for which in ("lmmse", "ideal"):
            twins = _twin(name, m, R, which)
            for s in (0, 1):                                                     # the CPU side: the twin alone stays within the cap
                share = float(twins[s][4][:, s].sum()) / max(2 * cfg.data_elements * G, 1)
                assert share <= SM_SHARE_CAP, (name, R, which, s, share)
                worst["flagged"] = max(worst["flagged"], share)
            for stride in (1, 2, 3):
                pattern, failed = _failed(G, shift=stride, stride=stride)
                assert failed.stride(0) == stride or G * 2 == 1
                redo = cwsic_redetect(pattern)
                counts, loss, llr, state = _run(name, m, R, failed, which)
                assert counts.shape == (2 * G, 2) and counts.dtype == torch.int32 and loss.shape == (2 * G, 3)
                assert llr.shape == (2 * G, *cfg.sim.ofdm, m) and state.shape == (G, 2) and state.dtype == torch.int32
                assert state.cpu().numpy().astype(bool).tolist() == redo.tolist() and int(state.max()) <= 1       # the truth table, exactly
                got, got_loss = counts.cpu().numpy().astype(np.int64).reshape(G, 2, 2), loss.cpu().numpy().astype(np.float64).reshape(G, 2, 3)
                got_llr = llr.cpu().numpy().astype(np.float64).reshape(G, 2, *cfg.sim.ofdm, m)
                assert not got[~redo].any() and not got_loss[~redo].any() and not got_llr[~redo].any()            # exactly zero
                assert np.isfinite(got_llr).all() and np.isfinite(got_loss).all() and (got >= 0).all()
                for g, s in zip(*np.nonzero(redo)):
                    want_counts, _, want_llr, _, flags, lo, hi, q = (v[g, s] for v in twins[s])
                    pairs, elems = int(flags.sum()), int(flags.any(axis=-1).sum())
                    assert abs(got[g, s, 0] - want_counts[0]) <= pairs and abs(got[g, s, 1] - want_counts[1]) <= elems, (name, R, which, g, s)
                    err = np.abs(got_llr[g, s] - want_llr)
                    assert (err <= e_l * q).all(), (name, R, which, g, s, float((err / np.where(q > 0, q, 1)).max()))
                    assert (lo * (1 - e_s) - FLOOR <= got_loss[g, s]).all() and (got_loss[g, s] <= hi * (1 + e_s) + FLOOR).all(), \
                        (name, R, which, g, s, got_loss[g, s], lo, hi)
                    rows += 1
                    differing += int((got[g, s] != want_counts).any())
                    if (q > 0).any():
                        worst["llr"] = max(worst["llr"], float((err[q > 0] / q[q > 0] / e_l).max()))
                    if pairs:
                        worst["bits"] = max(worst["bits"], abs(got[g, s, 0] - want_counts[0]) / pairs)
    assert rows > 0
    print(f"m = {m}: {differing} of {rows} re-detected (group, stream) rows differ from the definition in a count; largest |llr_dev - "
          f"llr_def| / (e_lambda_sic(R) q) = {worst['llr']:.2f}; largest bit-count difference / its allowance = {worst['bits']:.2f}; largest "
          f"flagged share of the twin {worst['flagged']:.2e}")


# ---- bit-for-bit identities ----

@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_stream_1_is_the_diversity_kernel_bit_for_bit(m):
    """``H_r1 = E_r1 = 0`` and the pattern (1, 0) in every group: stream 0 is ``LinkMrcPlan`` on the frames (r, 0); stream 1 is zeros."""
    f = _dev(FACTORS)
    for name, R, _ in sm_cases():
        cfg = LinkConfig(sm_inputs(name)[0], m)
        n, (ideal, est, keys, sigma, rho, scale), _ = _operands(name, R)
        G = n // (2 * R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        counts, loss, llr, state = _plan(name, m, R)(*(_dev(a) for a in (H, E, keys, sigma, rho, scale)), _every(G, 0), f, want_llr=True)
        want = LinkMrcPlan(cfg, DEV, R)(*(_dev(np.ascontiguousarray(a)) for a in (ideal[::2], est[::2], keys[::2], sigma[::2], rho[::2], scale)),
                                        f, want_llr=True)
        for got, w in zip((counts, loss, llr), want):
            assert torch.equal(got[0::2], w), (name, R)
        assert not llr[1::2].any() and not counts[1::2].any() and not loss[1::2].any() and state.tolist() == [[1, 0]] * G


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_second_stage_of_the_sic_kernel_after_a_correct_first_decision_bit_for_bit(m):
    """Outside the definition's dependent set the device's order and first decision are the definition's; where that first decision is
    the sent symbol, ``aft_link_sic_f32`` cancelled the very float32 this kernel cancels, by the same four fused multiply-adds."""
    compared = 0
    for name, R, n in sm_cases():
        cfg, G = LinkConfig(sm_inputs(name)[0], m), n // (2 * R)
        for which in ("lmmse", "ideal"):
            _, (ideal, est, keys, sigma, rho, scale, reg), dev = link2_gpu.operands("mmse", name, R, which)
            out = link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, 2, FACTORS, tau=derived_tau_sic(R))
            wrong, dep = out[4], out[6]
            first_s1 = _order(est, rho, R, cfg.sim.ofdm)                         # stream 1 is detected first: stream 0 second
            sic = LinkSicPlan(cfg, DEV, R)(*dev, _dev(FACTORS), want_llr=True)[2].reshape(G, 2, *cfg.sim.ofdm, m)
            for s in (0, 1):
                second = first_s1 if s == 0 else ~first_s1
                pick = second & cfg.data_mask[None] & (dep == 0) & (wrong[:, 1 - s] == 0)
                mine = _run(name, m, R, _every(G, s), which)[2].reshape(G, 2, *cfg.sim.ofdm, m)
                at = _dev(pick)
                assert torch.equal(mine[:, s][at], sic[:, s][at]), (name, R, which, s)
                compared += int(pick.sum())
    assert compared > 0
    print(f"m = {m}: {compared} (element, stream) pairs compared bit for bit with aft_link_sic_f32's second stage")


# ---- robustness of the cancel kernel ----

@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run(m):
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, snr, ideal, est = sm_inputs(name)
        for R in (2, 3):
            p, W = _plan(name, m, R), 2 * R
            idx = (np.arange(37 * W) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-W:] = np.arange(W, 2 * W)                                       # ... the last one group 1 of ``_operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est["lmmse"][i]), _dev(keys[i]), _dev(sigma[i]),  # noqa: E731
                             *(_dev(a) for a in sm_weights(snr[i], 0.0, R, 2, "mmse")[:2]))
            pattern, failed = _failed(37, shift=2)                               # group 36: pattern (38 mod 4) = (0, 1)
            assert pattern[36].tolist() == [0, 1]
            batch = p(*ops(idx), failed, f, want_llr=True)
            alone = p(*ops(np.arange(W, 2 * W)), _dev(np.asarray([0, 1], np.int32)), f, want_llr=True)
            _same_bits([t[72:74] for t in batch[:3]] + [batch[3][36:37]], alone)
            G = _operands(name, R)[0] // W
            whole = _run(name, m, R, _every(G, 1))
            _same_bits([t[2:4] for t in whole[:3]] + [whole[3][1:2]], alone)     # second of the groups of ``_operands``
            _same_bits(p(*ops(idx), failed, f, want_llr=True), batch)            # a second run of the same batch
            assert batch[2][72].abs().max() == 0 and batch[2][73].abs().max() > 0


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_poisoned_outputs_null_llr_null_state_and_bases_off_16_bytes(m):
    """Every element of the four outputs is written and nothing beside them -- in a group without a redo as well --; without the LLR
    output, without the state, and with ideal, est and llr 8, 4 and 12 bytes off a 16-byte boundary, the same bits."""
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        for R in (2, 3):
            n, _, ops = _operands(name, R)
            p, F, G = _plan(name, m, R), n // R, n // (2 * R)
            _, failed = _failed(G, shift=0, stride=3)                            # pattern (0, 0) first: a group that only stores zeros
            want = _run(name, m, R, failed)
            h, e = ops[0], ops[1]
            fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
            fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
            assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
            for hp, ep, off, with_state in ((None, None, 0, True), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8, True), (None, fe.data_ptr() + 8, 0, False),
                                            (None, None, 8, False), (None, None, 4, True), (fh.data_ptr() + 8, None, 12, True),
                                            (None, None, None, True), (None, None, None, False)):
                counts = torch.full((F + 1, 2), POISON, dtype=torch.int32, device=DEV)
                loss = torch.full((F + 1, 3), float("nan"), device=DEV)
                llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
                state = torch.full((G + 1, 2), POISON, dtype=torch.int32, device=DEV)
                _lib.check(_entry(p, ops, failed.data_ptr(), 3, f, counts, loss, None if off is None else llr.data_ptr() + off,
                                  state.data_ptr() if with_state else None, n, hp, ep))
                _same_bits([counts[:F], loss[:F]], want[:2])
                assert (counts[F:] == POISON).all() and loss[F:].isnan().all()
                if with_state:
                    _same_bits([state[:G]], [want[3]])
                    assert (state[G:] == POISON).all()
                else:
                    assert (state == POISON).all()
                if off is None:
                    assert llr.isnan().all()
                else:
                    at = off // 4
                    _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                    assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
            got = _run(name, m, R, failed, want_llr=False, want_state=False)
            assert got[2] is None and got[3] is None
            _same_bits(got[:2], want[:2])
    # the odd grid whose last element (14, at (2, 4)) is data and alone in its pair: written, finite and not a pilot's zero
    n, _, ops = _operands(MRC_ODD, 2)
    counts, state = (torch.full((2, 2), POISON, dtype=torch.int32, device=DEV), torch.full((1, 2), POISON, dtype=torch.int32, device=DEV))
    loss, llr = torch.full((2, 3), float("nan"), device=DEV), torch.full((2, 3, 5, m), float("nan"), device=DEV)
    _lib.check(_entry(_plan(MRC_ODD, m, 2), ops, _every(1, 1).data_ptr(), 1, f, counts, loss, llr.data_ptr(), state.data_ptr(), n))
    _same_bits([counts, loss, llr, state], _run(MRC_ODD, m, 2, _every(1, 1)))
    assert llr.isfinite().all() and (llr[1, 2, 4] != 0).all() and (llr[1, 1, 2] == 0).all() and not llr[0].any()


def test_failed_and_keys_in_pinned_host_memory_are_read_in_place():
    name, m, R = "odd_30x7", 4, 4
    n, (ideal, est, keys, sigma, rho, scale), ops = _operands(name, R)
    G = n // (2 * R)
    pattern, failed = _failed(G, shift=1, stride=2)
    want = _run(name, m, R, failed)
    wide = torch.full((2 * G, 2), POISON, dtype=torch.int32).pin_memory()
    wide[:, 1] = torch.from_numpy(pattern.reshape(-1))
    got = _plan(name, m, R)(ops[0], ops[1], _pinned(keys), ops[3], ops[4], ops[5], wide[:, 1], _dev(FACTORS), want_llr=True)
    torch.cuda.synchronize()
    _same_bits(got, want)


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_cancel_f32"):  # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_cancel_f32") and hasattr(lib, "aft_link_ldpc_masked_f32")
    for m in BITS_PER_SYMBOL:
        for name, R in (("default_120x14", 2), ("odd_30x7", 3), ("odd_30x7", 8), (MRC_ODD, 2)):
            G = _operands(name, R)[0] // (2 * R)
            for shift in (1, 2):
                failed = _failed(G, shift=shift)[1]
                _same_bits(_run(name, m, R, failed, lib=lib), _run(name, m, R, failed))
    for sim, m, rate in ((SIMS["odd_30x7"], 8, (3, 4)), (DEFAULT, 4, "1/2"), (DEFAULT, 8, (3, 4))):
        cfg, llr = ldpc_gpu._on(sim, m, rate)
        plan, mask = LinkLdpcPlan(cfg, DEV), _dev(np.asarray([1, 0, 1, 0, 1], np.int32))
        _same_bits(plan(llr, _dev(KEYS), want_bits=True, mask=mask, lib=lib), plan(llr, _dev(KEYS), want_bits=True, mask=mask))


def test_what_the_cancel_plan_refuses():
    n, _, (h, e, k, s, rho, scale) = _operands("odd_30x7", 4)
    p, f, G = _plan("odd_30x7", 4, 4), _dev(FACTORS), 4
    failed = _failed(G)[1]
    for args, word in (((h[:6], e[:6], k[:6], s[:6], rho[:6], scale, failed, f), "6 frames is not a multiple of branches \\* streams = 4 \\* 2"),
                       ((h, e, k, s, rho[:8], scale, failed, f), "rho must hold"), ((h, e, k, s, rho, scale[:3], failed, f), "scale must hold"),
                       ((h, e, k, s, rho, scale, failed[:3], f), "failed must hold one value per row \\(8\\)"),
                       ((h, e, k, s, rho, scale, failed.reshape(4, 2), f), "failed must hold one value per row"),
                       ((h, e, k, s, rho, scale, failed.long(), f), "failed must be torch.int32"),
                       ((h, e, k, s, rho, scale, torch.zeros(8, dtype=torch.int32), f), "pinned host memory"),
                       ((h, e, k, s, rho, scale, failed, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            p(*args)
    for bad in (0, 1, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            LinkCancelPlan(p.cfg, DEV, bad)
    for bad in (1, 3, 2.0, True):
        with pytest.raises(ValueError, match="streams"):
            LinkCancelPlan(p.cfg, DEV, 2, bad)
    with pytest.raises(ValueError, match="LinkCancelPlan runs on a HIP device"):
        LinkCancelPlan(p.cfg, "cpu", 2)


def test_every_refusal_of_the_cancel_entry_point_launches_nothing():
    name, m, R = "default_120x14", 4, 2
    n, _, (h, e, k, s, rho, scale) = _operands(name, R)
    lib, F, G, f = _lib.load(), n // R, n // (2 * R), _dev(FACTORS)
    fn = lib.aft_link_cancel_f32
    cfg = LinkConfig(sm_inputs(name)[0], m)
    failed = _failed(G, shift=1)[1]
    counts, state = (torch.full(shape, POISON, dtype=torch.int32, device=DEV) for shape in ((F, 2), (G, 2)))
    loss = torch.full((F, 3), float("nan"), device=DEV)
    llr = torch.full((F, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), rho=rho.data_ptr(), scale=scale.data_ptr(),
                factors=f.data_ptr(), n_factors=3, branches=R, streams=2, failed=failed.data_ptr(), failed_stride=1, counts=counts.data_ptr(),
                loss=loss.data_ptr(), llr=llr.data_ptr(), state=state.data_ptr(), batch=n)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return fn(ctypes.byref(p), *(a[x] for x in good), None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error(), kw)

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert fn(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for x in ("ideal", "est", "keys", "sigma", "rho", "scale", "factors", "failed", "counts", "loss"):
        refused(E, "NULL pointer", **{x: None})
    for x in ("ideal", "est", "keys"):
        refused(E, "8-byte", **{x: good[x] + 4})
    for x in ("sigma", "rho", "scale", "factors", "failed", "counts", "loss", "llr", "state"):
        refused(E, "4-byte", **{x: good[x] + 2})
    for stride in (0, -1, -3):
        refused(E, f"failed_stride must be at least 1 (got {stride})", failed_stride=stride)
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
    for field, value, word in (("num_scs", 0, "num_scs = 0"), ("pilot_scs", 65, "pilot_scs = 65 is outside 1..64"),
                               ("num_symbols", 1, "larger than the ofdm grid"), ("bits_per_symbol", 3, "bits_per_symbol = 3")):
        p = cfg.to_struct()
        setattr(p, field, value)
        refused(SH, word, p=p)
    torch.cuda.synchronize()
    assert (counts == POISON).all() and loss.isnan().all() and llr.isnan().all() and (state == POISON).all()     # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    _same_bits([counts, loss, llr, state], _run(name, m, R, failed))             # ... and the good call writes it all
    # a grid whose every element is a pilot is legal: counts 0, loss 0, LLR 0, the flags as the table has them
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    assert call(one, batch=4) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert counts[:2].tolist() == [[0, 0]] * 2 and loss[:2].tolist() == [[0.0] * 3] * 2 and llr.reshape(-1)[:2 * m].tolist() == [0.0] * (2 * m)
    assert state[0].tolist() == [1, 0]


# ---- the masked decoder ----

def _masks(b):
    return {"ones": np.ones(b, np.int32), "zeros": np.zeros(b, np.int32), "alternating": (np.arange(b) % 2).astype(np.int32),
            "counts": np.asarray([(-5, 0, 7, 0, 1 << 30)[i % 5] for i in range(b)], np.int32)}      # any non-zero word selects


def _strided(mask, stride):
    wide = torch.full((len(mask), stride), POISON, dtype=torch.int32, device=DEV)
    wide[:, 0] = _dev(mask)
    return wide[:, 0]


def _masked_poisoned(cfg, llr, keys, mask, stride, want_bits=True, lib=None):
    """The entry point itself on outputs filled with values no decoder writes."""
    lib = lib or _lib.load()
    b = llr.shape[0]
    counts = torch.full((b + 1, 3), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((b + 1, cfg.blocks, cfg.info_bits), 0xAB, dtype=torch.uint8, device=DEV)
    shifts = np.ascontiguousarray(cfg.shifts, dtype=np.int32)
    _lib.check(lib.aft_link_ldpc_masked_f32(ctypes.byref(cfg.link.to_struct()), llr.data_ptr(), keys.data_ptr(), cfg.base_rows, cfg.base_cols,
                                            shifts.ctypes.data, cfg.stride, cfg.stride_inverse, cfg.qgain, cfg.offset, cfg.max_iters,
                                            mask.data_ptr(), stride, counts.data_ptr(), bits.data_ptr() if want_bits else None, b,
                                            _lib.current_stream_ptr(llr.device)), lib)
    assert (counts[b:] == -7).all() and (bits[b:] == 0xAB).all()                 # nothing beside the outputs
    return counts[:b], bits[:b]


def _masked_equal_to_the_host(cfg, llr, lib=None):
    """Selected frames are ``link_ldpc_host``'s, the others zeros, for every mask and stride; all ones is ``aft_link_ldpc_f32`` bit for bit."""
    want_counts, want_bits = link_ldpc_host(cfg, KEYS, llr.cpu().numpy())
    plain = LinkLdpcPlan(cfg, DEV)(llr, _dev(KEYS), want_bits=True, lib=lib)
    assert plain[0].cpu().tolist() == want_counts.tolist()
    for tag, mask in _masks(FRAMES).items():
        for stride in (1, 2):
            view = _strided(mask, stride)
            counts, bits = _masked_poisoned(cfg, llr, _dev(KEYS), view, stride, lib=lib)
            on = mask != 0
            assert counts.cpu().numpy()[on].tolist() == want_counts[on].tolist() and not counts.cpu().numpy()[~on].any(), (tag, stride)
            assert np.array_equal(bits.cpu().numpy()[on], want_bits[on]) and not bits.cpu().numpy()[~on].any(), (tag, stride)
            bare, untouched = _masked_poisoned(cfg, llr, _dev(KEYS), view, stride, want_bits=False, lib=lib)     # bits = NULL: the same counts
            assert torch.equal(bare, counts) and (untouched == 0xAB).all()
            if tag == "ones":
                assert torch.equal(counts, plain[0]) and torch.equal(bits, plain[1])
            by_plan = LinkLdpcPlan(cfg, DEV)(llr, _dev(KEYS), want_bits=True, mask=view, lib=lib)
            assert torch.equal(by_plan[0], counts) and torch.equal(by_plan[1], bits)


def test_masked_decoder_on_the_smallest_code_one_block_and_six():
    for m in (2, 8):
        cfg, llr = ldpc_gpu._on(SIMS["odd_30x7"], m, (3, 4))
        assert cfg.blocks == (1 if m == 2 else 6)
        _masked_equal_to_the_host(cfg, llr)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_masked_decoder_on_a_rate_preset_at_every_order(m):
    cfg, llr = ldpc_gpu._on(DEFAULT, m, ("1/2", "2/3", "3/4", "1/2")[m // 2 - 1])
    assert cfg.blocks == m
    _masked_equal_to_the_host(cfg, llr)


def test_masked_decoder_with_more_blocks_than_waves():
    cfg, llr = ldpc_gpu._on(DEFAULT, 8, (3, 4))
    assert cfg.blocks == 51
    _masked_equal_to_the_host(cfg, llr)


def test_a_masked_frame_does_not_depend_on_its_batch_its_position_or_the_run():
    cfg, five = ldpc_gpu._on(SIMS["odd_30x7"], 8, (4, 6))
    plan = LinkLdpcPlan(cfg, DEV)
    order = [3, 0, 4, 4, 1, 2, 0, 0, 3, 1, 2]
    mask = np.asarray([1, 1, 0, 1, 1, 1, 0, 1, 0, 0, 1], np.int32)
    llr, keys = five[order].contiguous(), _dev(KEYS[order])
    counts, bits = plan(llr, keys, want_bits=True, mask=_dev(mask))
    alone = [plan(five[i:i + 1], _dev(KEYS[i:i + 1]), want_bits=True) for i in range(FRAMES)]
    for at, i in enumerate(order):
        if mask[at]:
            assert torch.equal(counts[at:at + 1], alone[i][0]) and torch.equal(bits[at:at + 1], alone[i][1])
        else:
            assert not counts[at].any() and not bits[at].any()
    again = plan(llr, keys, want_bits=True, mask=_dev(mask))
    assert torch.equal(again[0], counts) and torch.equal(again[1], bits)
    pinned = torch.from_numpy(mask).pin_memory()                                 # the mask in pinned host memory, read in place
    got = plan(llr, keys, want_bits=True, mask=pinned)
    torch.cuda.synchronize()
    assert torch.equal(got[0], counts) and torch.equal(got[1], bits)
    for bad, word in ((_dev(mask)[:3], "mask must hold one value per row \\(11\\)"), (_dev(mask).long(), "mask must be torch.int32"),
                      (torch.from_numpy(mask), "pinned host memory"), (_dev(mask).reshape(11, 1), "mask must hold one value per row")):
        with pytest.raises(ValueError, match=word):
            plan(llr, keys, mask=bad)


@pytest.mark.parametrize("value", (float("nan"), 1e30))
def test_the_masked_bits_do_not_depend_on_what_the_lds_held(value):
    for sim, m, rate in ((SIMS["odd_30x7"], 8, (3, 4)), (DEFAULT, 4, "1/2"), (DEFAULT, 8, (3, 4))):
        cfg, llr = ldpc_gpu._on(sim, m, rate)
        plan, mask = LinkLdpcPlan(cfg, DEV), _dev(np.asarray([1, 0, 1, 1, 0], np.int32))
        want = plan(llr, _dev(KEYS), want_bits=True, mask=mask)
        fill_lds(value, "cuda:0")
        got = plan(llr, _dev(KEYS), want_bits=True, mask=mask)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_every_refusal_of_the_masked_entry_point_launches_nothing():
    cfg, llr = ldpc_gpu._on(SIMS["odd_30x7"], 4, (3, 5))
    lib = _lib.load()
    keys, mask = _dev(KEYS), _dev(np.ones(FRAMES, np.int32))
    counts = torch.full((FRAMES, 3), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((FRAMES, 2, 128), 0xAB, dtype=torch.uint8, device=DEV)
    table = np.ascontiguousarray(cfg.shifts, dtype=np.int32)
    good = dict(llr=llr.data_ptr(), keys=keys.data_ptr(), base_rows=3, base_cols=5, shifts=table.ctypes.data, stride=cfg.stride,
                stride_inverse=cfg.stride_inverse, qgain=8.0, offset=4, max_iters=20, mask=mask.data_ptr(), mask_stride=1,
                counts=counts.data_ptr(), bits=bits.data_ptr(), batch=FRAMES)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.link.to_struct() if p is None else p
        return lib.aft_link_ldpc_masked_f32(ctypes.byref(p), *(a[n] for n in good), None)

    def refused(rc_want, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == rc_want and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error(), kw)

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_ldpc_masked_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for name in ("llr", "keys", "shifts", "mask", "counts"):
        refused(E, "link ldpc masked: NULL pointer", **{name: None})
    refused(E, "8-byte", keys=good["keys"] + 4)
    for name in ("llr", "shifts", "mask", "counts"):
        refused(E, "4-byte", **{name: good[name] + 2})
    for stride in (0, -1):
        refused(E, f"mask_stride must be at least 1 (got {stride})", mask_stride=stride)
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for qgain in (0.0, float("nan")):
        refused(E, "finite and positive", qgain=qgain)
    refused(SH, "base_rows = 2 is outside 3..16", base_rows=2)
    refused(SH, "base_cols = 33 is outside 4..32", base_cols=33)
    refused(SH, "offset = 128 is outside 0..127", offset=128)
    refused(SH, "max_iters = 0 is outside 1..255", max_iters=0)
    refused(SH, "is outside [1, 640)", stride=640)
    refused(SH, "not coprime", stride=5)
    refused(SH, "is not the inverse", stride_inverse=1)
    p = cfg.link.to_struct()
    p.bits_per_symbol = 3
    refused(SH, "bits_per_symbol = 3", p=p)
    torch.cuda.synchronize()
    assert (counts == -7).all() and (bits == 0xAB).all()                         # nothing was launched
    assert call() == _abi.AFT_OK and call(bits=None) == _abi.AFT_OK
    torch.cuda.synchronize()
    want_counts, want_bits = link_ldpc_host(cfg, KEYS, llr.cpu().numpy())
    assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))


# ---- the chain end to end ----

def _chain(code, R, keys, sigma, snr, ideal, est):
    """The four launches on the device and every integer stage again on the host, fed the device's own float32 LLRs: ``(first, redo,
    second, final)`` int64 / bool ``[G, 2, ...]`` from the device, each asserted equal to the host's."""
    link, G = code.link, len(keys) // (2 * R)
    rho, scale, reg = (_dev(a) for a in sm_weights(snr, 0.0, R, 2, "mmse"))
    ops = (_dev(ideal), _dev(est), _dev(keys), _dev(sigma), rho, scale)
    one = torch.ones(1, device=DEV)
    sent = np.ascontiguousarray(keys.reshape(G, R, 2)[:, 0, :]).reshape(-1)
    decode = LinkLdpcPlan(code, DEV)
    llr1 = LinkSmPlan(link, DEV, R)(*ops, reg, one, want_llr=True)[2]
    first = decode(llr1, _dev(sent))[0]
    _, _, llr2, state = LinkCancelPlan(link, DEV, R)(*ops, first[:, 1], one, want_llr=True)    # the decoder's block errors, in place
    second = decode(llr2, _dev(sent), mask=state.view(-1))[0]
    first, second, redo = first.cpu().numpy().astype(np.int64), second.cpu().numpy().astype(np.int64), state.cpu().numpy().astype(bool)
    want_first = link_ldpc_host(code, sent, llr1.cpu().numpy())[0]
    assert np.array_equal(first, want_first)                                      # first-pass counts
    want_redo = cwsic_redetect(want_first[:, 1].reshape(G, 2))
    assert np.array_equal(redo, want_redo)                                        # state
    pick = want_redo.reshape(-1)
    want_second = np.zeros_like(want_first)
    if pick.any():
        want_second[pick] = link_ldpc_host(code, sent[pick], llr2.cpu().numpy()[pick])[0]
    assert np.array_equal(second, want_second) and not llr2[_dev(~pick)].any()     # second-pass counts; no LLR where nothing is detected again
    first, second = first.reshape(G, 2, 3), second.reshape(G, 2, 3)
    return first, redo, second, cwsic_final(first, redo, second)


def _accumulated(code, R, seed, ids, snr, ideal, est, batch):
    acc = LdpcBlockErrorAccumulator(code, DEV, seed=seed, branches=R, streams=2, detector="cwsic")
    assert type(acc._plan) is LinkSmPlan and type(acc._cancel) is LinkCancelPlan
    for lo in range(0, len(ids), batch):
        sl = slice(lo, lo + batch)
        acc.update(None if est is None else _dev(est[sl]), _dev(ideal[sl]), frame_ids=ids[sl], snr_db=snr[sl])
    return acc


def _results_are(acc, code, first, redo, second, final):
    F, B = redo.size, code.blocks
    again, decoded = int(redo.sum()), int((redo & (second[..., 1] == 0)).sum())
    assert acc.frames == F and acc.errors.is_cuda and acc.errors.cpu().tolist() == final.sum(axis=(0, 1)).tolist()
    assert acc.result() == final[..., 1].sum() / (F * B) and acc.result_first_pass() == first[..., 1].sum() / (F * B)
    assert acc.result_ber() == final[..., 0].sum() / (F * code.info_bits_per_frame) and acc.result_iterations() == final[..., 2].sum() / (F * B)
    assert acc.result_throughput() == (F * B - final[..., 1].sum()) * code.info_bits / (F * code.link.data_elements)
    assert acc.cwsic_stats() == (again / F, decoded / again if again else 0.0, int((first[..., 1] > 0).all(axis=1).sum()) / (F // 2))


def test_the_chain_on_the_physical_inputs_and_the_orderings_on_the_device():
    """Every integer stage is exact against the host definition on the device's own LLRs; the accumulator's results are that
    recomputation; and the physical conditions of tests/test_linkcwsic.py hold on the device's own counts."""
    code, keys, sigma, snr, ideal, est = physical_inputs()
    R, seed = PHYSICAL["branches"], PHYSICAL["key_seed"]
    counts = {}
    for which, e in est.items():
        counts[which] = _chain(code, R, keys, sigma, snr, ideal, e)
        acc = _accumulated(code, R, seed, np.arange(len(keys)), snr, ideal, None if which == "perfect" else e, 64)
        _results_are(acc, code, *counts[which])
    physical_conditions(counts)


@pytest.mark.parametrize("m", (2, 8))
def test_the_chain_on_the_odd_grid_with_the_smallest_code(m):
    code = LdpcConfig(LinkConfig(SIMS["odd_30x7"], m), (3, 4))                    # one block at m = 2, six at m = 8
    for R in (2, 4):
        sim, keys, sigma, snr, ideal, est = sm_inputs("odd_30x7")
        n = len(keys) // (2 * R) * 2 * R
        got = _chain(code, R, keys[:n], sigma[:n], snr[:n], ideal[:n], est["lmmse"][:n])
        print(f"m = {m}, R = {R}: {int((got[0][..., 1] > 0).sum())} streams failed, {int(got[1].sum())} detected again")


def test_a_sweep_from_the_loader_runs_without_a_synchronisation():
    """Three batches from ``SynthLoader``, the last two under the no-synchronisation guard; the sums are the four launches' of each
    batch, recomputed with the plans, and keys hashed on the device give the same sums."""
    R, N, seed = 2, 2, 2
    sim = ChannelSimConfig()
    link = LinkConfig(sim, 2)
    code = LdpcConfig(link, "3/4")
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    with_est, perfect, on_device = (LdpcBlockErrorAccumulator(code, DEV, seed=seed, branches=R, streams=N, detector="cwsic") for _ in range(3))
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
    assert len(seen) == 3 and with_est.frames == perfect.frames == 48 // R and with_est.errors.is_cuda
    parts = [[], []]
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1).astype(np.float64)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        for i, e in enumerate((est, ideal)):
            parts[i].append(_chain(code, R, keys, noise_sigma(snr), snr, ideal.cpu().numpy(), e.cpu().numpy()))
    for acc, got in ((with_est, parts[0]), (perfect, parts[1]), (on_device, parts[0])):
        _results_are(acc, code, *(np.concatenate([p[k] for p in got]) for k in range(4)))
    print(f"QPSK rate 3/4, 2 x 2: BLER {with_est.result_first_pass():.3f} -> {with_est.result():.3f} with the LMMSE estimate, "
          f"{perfect.result_first_pass():.3f} -> {perfect.result():.3f} with the channel; stats {with_est.cwsic_stats()} / {perfect.cwsic_stats()}")
