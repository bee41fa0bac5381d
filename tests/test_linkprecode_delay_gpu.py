"""``aft_link_precoded_delayed_f32``, ``hip_ops.LinkPrecodedPlan(..., slots=, delay=)`` and the ``precoding_delay=`` argument of the
accumulators on the HIP device: ``delay=0`` against ``aft_link_precoded_f32`` bit for bit, estimates made equal across a sequence's slots
against it on the transmit groups bit for bit, the applied PMIs against its PMIs on the feedback groups bit for bit, the general case
against the float64 twin, a NULL ``llr``, bases off 16 bytes, poisoned outputs, the checked build, every refusal, and
``LinkAccumulator`` / ``LdpcBlockErrorAccumulator`` with ``precoding_delay=1`` without a synchronisation against the host path on the
device's own LLRs.

The general comparison is tests/test_linkprecode_gpu.py's, flag for flag: the delayed kernel is the same walk with two group numbers,
so the arithmetic per element and per subband is unchanged and that file's ``derived_tau_pmi``, ``derived_tau(R)``,
``derived_e_lambda(R)``, ``derived_e_s`` and its caps (at most one PMI-flagged subband and one flagged decision per case on the small
grid, ``SHARE_CAP`` of the decisions on the large one) carry over as they stand; they are imported, not restated.  The device's PMIs are
compared with the twin's outside PMI-flagged subbands, and everything downstream with the twin EVALUATED WITH THE DEVICE'S PMIs.  The
observed flagged share is printed.

The inputs are tests/test_linkprecode_delay.py's ``delay_inputs``: 24 frames of 30 x 7 and of 3 x 5."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkPrecodedPlan
from adafortitran_amd.linksim import (LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, delayed_groups, link_ldpc_host,
                                      link_precoded_host, noise_sigma, precoding_pmi_host, precoding_weights)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linkmrc import MRC_ODD
from test_linkprecode import PMI_TAU_CAP
from test_linkprecode_delay import DELAY_SIMS, EQUAL_SNR, FRAMES, MIXED_SNR, delay_operands, equal_estimates
from test_linkprecode_gpu import FACTORS, POISON, derived_e_lambda, derived_tau, derived_tau_pmi
from test_linksim import SHARE_CAP, flagged_share
from test_linksim_gpu import _dev
from test_linksoft_gpu import FLOOR, derived_e_s

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(name, R, m, B) for name in DELAY_SIMS for R in (1, 2) for m in (2, 6) for B in (1, 7, None)]
_ops = {}


def _band(name, B):
    S = DELAY_SIMS[name].ofdm[0]
    return S if B is None else min(B, S)


def _operands(name, R, which=MIXED_SNR, equal=False):
    """(host, device) tuples (ideal, est, keys, sigma, rho, scale) in the order the plan takes them; ``equal``: every slot of a
    sequence of three has slot 0's estimate."""
    if (name, R, which, equal) not in _ops:
        sim, keys, sigma, ideal, est, rho, scale = delay_operands(name, R, which)
        host = (ideal, equal_estimates(est, R, 3) if equal else est, keys, sigma, rho, scale)
        _ops[name, R, which, equal] = (host, tuple(_dev(np.ascontiguousarray(a)) for a in host))
    return _ops[name, R, which, equal]


def _plan(name, m, R, B, slots=1, delay=0):
    return LinkPrecodedPlan(LinkConfig(DELAY_SIMS[name], m), DEV, R, B, slots, delay)


def _rows(ops, groups, width):
    """The operands of the given groups of ``width`` frames (the per-group scale by group)."""
    at = (torch.as_tensor(groups, device=DEV)[:, None] * width + torch.arange(width, device=DEV)[None, :]).reshape(-1)
    return tuple(t[at].contiguous() for t in ops[:5]) + (ops[5][torch.as_tensor(groups, device=DEV)].contiguous(),)


@pytest.mark.parametrize("name,R,m,B", CASES)
def test_no_delay_is_the_instantaneous_kernel_bit_for_bit(name, R, m, B):
    B, f = _band(name, B), _dev(FACTORS)
    _, ops = _operands(name, R)
    want = _plan(name, m, R, B)(*ops, f, want_llr=True)
    lib, G = _lib.load(), FRAMES // (2 * R)
    for K in (1, 3):                                            # slots = 1 through the entry point itself: the plan takes the sibling there
        counts = torch.full((G, 2), POISON, dtype=torch.int32, device=DEV)
        loss = torch.full((G, 3), float("nan"), device=DEV)
        llr = torch.full_like(want[2], float("nan"))
        pmi = torch.full_like(want[3], POISON)
        p = _plan(name, m, R, B)
        _lib.check(lib.aft_link_precoded_delayed_f32(ctypes.byref(p.link), *(t.data_ptr() for t in ops), f.data_ptr(), 3, R, B, K, 0,
                                                     counts.data_ptr(), loss.data_ptr(), llr.data_ptr(), pmi.data_ptr(), FRAMES,
                                                     _lib.current_stream_ptr(counts.device)))
        _same_bits([counts, loss, llr, pmi], want)
    _same_bits(_plan(name, m, R, B, 3, 0)(*ops, f, want_llr=True), want)


@pytest.mark.parametrize("name,R,m,B", CASES)
def test_equal_estimates_and_the_feedback_groups_pmis_bit_for_bit(name, R, m, B):
    B, f, K, W = _band(name, B), _dev(FACTORS), 3, 2 * R
    instant = _plan(name, m, R, B)
    # equal estimates (and equal rho) across a sequence's slots: delay 1 is the instantaneous kernel on the transmit groups
    _, ops = _operands(name, R, EQUAL_SNR, equal=True)
    sent, _ = delayed_groups(FRAMES // W, K, 1)
    _same_bits(_plan(name, m, R, B, K, 1)(*ops, f, want_llr=True), instant(*_rows(ops, sent, W), f, want_llr=True))
    # the general case: the applied PMIs are the instantaneous kernel's on the feedback groups
    _, ops = _operands(name, R)
    every = instant(*ops, f)[3]
    for d in (1, 2):
        sent, feedback = delayed_groups(FRAMES // W, K, d)
        got = _plan(name, m, R, B, K, d)(*ops, f)
        assert got[3].shape == (len(sent), -(-DELAY_SIMS[name].ofdm[0] // B)) and got[2] is None
        _same_bits([got[3]], [every[torch.as_tensor(feedback, device=DEV)]])


@pytest.mark.parametrize("K,d", [(3, 1), (3, 2)])
@pytest.mark.parametrize("name,R,m,B", CASES)
def test_delayed_kernel_against_the_float64_twin(name, R, m, B, K, d):
    B = _band(name, B)
    cfg = LinkConfig(DELAY_SIMS[name], m)
    (S, T), W = cfg.sim.ofdm, 2 * R
    e_s, e_l, tau = derived_e_s(cfg), derived_e_lambda(R), derived_tau(R)
    tau_pmi = derived_tau_pmi(min(B, S) * T, R, -(-S // B))
    assert tau_pmi <= PMI_TAU_CAP
    (ideal, est, keys, sigma, rho, scale), ops = _operands(name, R)
    counts, loss, llr, pmi = _plan(name, m, R, B, K, d)(*ops, _dev(FACTORS), want_llr=True)
    rows, n_sub = FRAMES // W // K * (K - d), -(-S // B)
    assert counts.shape == (rows, 2) and counts.dtype == torch.int32 and loss.shape == (rows, 3) and llr.shape == (rows, S, T, m)
    assert pmi.shape == (rows, n_sub) and pmi.dtype == torch.int32
    got_pmi = pmi.cpu().numpy()
    want_pmi, pflags = precoding_pmi_host(cfg, est, rho, R, B, tau_pmi, slots=K, delay=d)
    assert got_pmi.min() >= 0 and got_pmi.max() <= 3 and pflags.sum() <= 1
    assert np.array_equal(got_pmi[~pflags], want_pmi[~pflags])
    want_counts, _, want_llr, _, flags, lo, hi, q, _ = link_precoded_host(cfg, keys, ideal, est, sigma, rho, scale, R, B, FACTORS, tau=tau,
                                                                         e_lambda=e_l, pmi=got_pmi, slots=K, delay=d)
    share = flagged_share(cfg, flags)
    if name == MRC_ODD:
        assert flags.sum() <= 1, int(flags.sum())
    else:
        assert share <= SHARE_CAP, share
    got = counts.cpu().numpy().astype(np.int64)
    pairs, elems = flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2))
    assert (got >= 0).all() and (np.abs(got[:, 0] - want_counts[:, 0]) <= pairs).all(), (got, want_counts, pairs)
    assert (np.abs(got[:, 1] - want_counts[:, 1]) <= elems).all(), (got, want_counts, elems)
    got_llr = llr.cpu().numpy().astype(np.float64)
    err = np.abs(got_llr - want_llr)
    ratio = float((err[q > 0] / q[q > 0] / e_l).max()) if (q > 0).any() else 0.0
    assert np.isfinite(got_llr).all() and (err <= e_l * q).all(), ratio
    got_loss = loss.cpu().numpy().astype(np.float64)
    assert np.isfinite(got_loss).all() and (lo * (1 - e_s) - FLOOR <= got_loss).all() and (got_loss <= hi * (1 + e_s) + FLOOR).all()
    print(f"  {name} R = {R} m = {m} B = {B} K = {K} d = {d}: {int(pflags.sum())} of {pflags.size} subbands PMI-flagged, "
          f"{int((got_pmi != want_pmi).sum())} PMIs differ; flagged share {share:.2e}; {int((got != want_counts).any(axis=1).sum())} of "
          f"{rows} rows differ from the definition; |llr_dev - llr_def| / (e_lambda q) = {ratio:.3f}")


@pytest.mark.parametrize("m", (2, 6))
def test_poisoned_outputs_a_null_llr_and_bases_off_16_bytes(m):
    """Every element of the four COMPACT outputs is written and nothing beside them; without the LLR output, and with ideal, est and
    llr off a 16-byte boundary, the same bits."""
    f, K, d = _dev(FACTORS), 3, 1
    for name, R, B in (("odd_30x7", 2, 7), ("odd_30x7", 1, 30), (MRC_ODD, 2, 1)):
        _, ops = _operands(name, R)
        p = _plan(name, m, R, B, K, d)
        want = p(*ops, f, want_llr=True)
        rows = FRAMES // (2 * R) // K * (K - d)
        assert want[0].shape[0] == rows and want[2].isfinite().all()
        h, e = ops[0], ops[1]
        fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
        fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
        assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
        for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (None, fe.data_ptr() + 8, 4), (fh.data_ptr() + 8, None, 12),
                            (None, None, None)):
            counts = torch.full((rows + 1, 2), POISON, dtype=torch.int32, device=DEV)
            loss = torch.full((rows + 1, 3), float("nan"), device=DEV)
            llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
            pmi = torch.full((rows + 1, p.n_sub), POISON, dtype=torch.int32, device=DEV)
            _lib.check(_lib.load().aft_link_precoded_delayed_f32(
                ctypes.byref(p.link), hp or h.data_ptr(), ep or e.data_ptr(), *(t.data_ptr() for t in ops[2:]), f.data_ptr(), 3, R, B, K, d,
                counts.data_ptr(), loss.data_ptr(), None if off is None else llr.data_ptr() + off, pmi.data_ptr(), FRAMES,
                _lib.current_stream_ptr(counts.device)))
            _same_bits([counts[:rows], loss[:rows], pmi[:rows]], [want[0], want[1], want[3]])
            assert (counts[rows:] == POISON).all() and loss[rows:].isnan().all() and (pmi[rows:] == POISON).all()
            if off is None:
                assert llr.isnan().all()
            else:
                at = off // 4
                _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
        got = p(*ops, f, want_llr=False)
        assert got[2] is None
        _same_bits([got[0], got[1], got[3]], [want[0], want[1], want[3]])
        _same_bits(p(*ops, f, want_llr=True), want)                              # a second run


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_precoded_delayed_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_precoded_delayed_f32")
    f = _dev(FACTORS)
    for name, R, m, B in CASES:
        B = _band(name, B)
        for K, d in ((3, 0), (3, 1), (3, 2)):
            p = _plan(name, m, R, B, K, d)
            _, ops = _operands(name, R)
            _same_bits(p(*ops, f, want_llr=True, lib=lib), p(*ops, f, want_llr=True))


def test_what_the_plan_refuses():
    name, R, B = "odd_30x7", 2, 7
    _, (h, e, k, s, rho, scale) = _operands(name, R)
    cfg, f = LinkConfig(DELAY_SIMS[name], 4), _dev(FACTORS)
    for slots, delay in ((0, 0), (3, 3), (3, -1), (1, 1), (2.0, 1), (3, True), (True, 0)):
        with pytest.raises(ValueError, match="slots"):
            LinkPrecodedPlan(cfg, DEV, R, B, slots, delay)
    p = LinkPrecodedPlan(cfg, DEV, R, B, 3, 1)
    with pytest.raises(ValueError, match="16 frames is not a multiple of slots \\* 2 \\* branches = 3 \\* 2 \\* 2"):
        p(h[:16], e[:16], k[:16], s[:16], rho[:16], scale[:4], f)
    with pytest.raises(ValueError, match="scale must hold"):
        p(h, e, k, s, rho, scale[:4], f)                        # scale is per INPUT group: 6
    assert p(h, e, k, s, rho, scale, f)[0].shape == (4, 2)


def test_every_refusal_of_the_entry_point_launches_nothing():
    """Every refusal of this entry point is AFT_ERR_ARG: ``aft_link_precoded_f32``'s, then the slots, the delay and the batch."""
    name, m, R, B, K, d = "odd_30x7", 4, 2, 7, 3, 1
    _, (h, e, k, s, rho, scale) = _operands(name, R)
    lib, rows, f = _lib.load(), FRAMES // (2 * R) // K * (K - d), _dev(FACTORS)
    fn = lib.aft_link_precoded_delayed_f32
    cfg = LinkConfig(DELAY_SIMS[name], m)
    counts = torch.full((FRAMES, 2), POISON, dtype=torch.int32, device=DEV)      # room for every good call below
    loss = torch.full((FRAMES, 3), float("nan"), device=DEV)
    llr = torch.full((FRAMES, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    pmi = torch.full((FRAMES, 30), POISON, dtype=torch.int32, device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), rho=rho.data_ptr(), scale=scale.data_ptr(),
                factors=f.data_ptr(), n_factors=3, branches=R, subband=B, slots=K, delay=d, counts=counts.data_ptr(), loss=loss.data_ptr(),
                llr=llr.data_ptr(), pmi=pmi.data_ptr(), batch=FRAMES)

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
    for field, value, word in (("num_scs", 0, "num_scs = 0"), ("num_symbols", -1, "num_symbols = -1"), ("pilot_scs", 65, "pilot_scs = 65"),
                               ("bits_per_symbol", 3, "bits_per_symbol = 3")):
        p = cfg.to_struct()
        setattr(p, field, value)
        refused(word, p=p)
    for bad in (0, 9, -2):
        refused(f"branches = {bad} is outside 1..8", branches=bad)
    for bad in (0, 31, -1):
        refused(f"subband = {bad} is outside 1..30", subband=bad)
    refused("batch = 22 is not a multiple of branches * 2 = 2 * 2", batch=22)
    p = cfg.to_struct()
    p.num_scs = 2048
    refused("subband = 1 makes 2048 subbands of the 2048 subcarriers, more than 1024", p=p, subband=1)
    for bad in (0, -1):
        refused(f"slots must be at least 1 (got {bad})", slots=bad)
    for bad in (3, -1, 7):
        refused(f"delay = {bad} is outside 0 .. slots - 1 = 2", delay=bad)
    refused("delay = 1 is outside 0 .. slots - 1 = 0", slots=1)
    refused("batch = 24 is not a multiple of slots * 2 * branches = 4 * 2 * 2", slots=4)
    refused("batch = 20 is not a multiple of slots * 2 * branches = 3 * 2 * 2", batch=20)
    torch.cuda.synchronize()
    assert (counts == POISON).all() and loss.isnan().all() and llr.isnan().all() and (pmi == POISON).all()     # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    want = _plan(name, m, R, B, K, d)(h, e, k, s, rho, scale, f, want_llr=True)
    _same_bits([counts[:rows], loss[:rows], llr[:rows], pmi.reshape(-1)[:rows * 5]], [*want[:3], want[3].reshape(-1)])
    assert (counts[rows:] == POISON).all() and llr[rows:].isnan().all() and (pmi.reshape(-1)[rows * 5:] == POISON).all()


def test_accumulators_with_delayed_feedback_run_without_a_synchronisation():
    """``precoding_delay=1, slots=3`` at 2 x 2 on sequences the simulator makes on the device: the batches run without a
    synchronisation, one link launch each; the errors and the histogram of the APPLIED PMIs are the plan's own, the LDPC accumulator's
    counts the host decoder's on the device's own LLRs with the leader keys of the transmit slots, and the host path
    (``link_precoded_host``) on the same frames gives the twin's counts within the flagged decisions."""
    R, seed, B, K, d = 2, 2, 12, 3, 1
    sim = ChannelSimConfig(slots=K, antennas=(R, 2), rx_correlation=0.4)
    link = LinkConfig(sim, 4)
    code = LdpcConfig(link, "1/2")
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 24, 24 * 3, device=DEV, seed=seed)                 # two sequences a batch
    kw = dict(seed=seed, branches=R, precoding_subband=B, precoding_delay=d, slots=K)
    hard, ldpc, on_device = LinkAccumulator(link, DEV, **kw), LdpcBlockErrorAccumulator(code, DEV, **kw), LinkAccumulator(link, DEV, **kw)
    assert all(type(a._plan) is LinkPrecodedPlan and (a._plan.slots, a._plan.delay) == (K, d) for a in (hard, ldpc))
    instant = LinkAccumulator(link, DEV, seed=seed, branches=R, precoding_subband=B, slots=K)
    assert (instant._plan.slots, instant._plan.delay) == (1, 0)                  # no delay: the instantaneous launch, whatever slots
    it = iter(loader)
    seen = []

    def step(batch):
        pil, ideal, meta = batch
        est = model(pil, meta)
        for acc in (hard, ldpc, instant):
            acc.update(est, ideal, meta)
        on_device.update(est, ideal, frame_ids=meta[0].to(DEV, non_blocking=True), snr_db=meta[1])
        seen.append((ideal, est, meta))

    step(next(it))                                # the first batch builds the plans and the pinned blocks: outside the guard
    torch.cuda.synchronize()
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                          # the mode is honoured: what follows is not vacuous
        for batch in it:
            step(batch)
    groups = 3 * 2 * (K - d)
    assert len(seen) == 3 and hard.frames == ldpc.frames == on_device.frames == groups and instant.frames == 3 * 2 * K
    p, one = LinkPrecodedPlan(link, DEV, R, B, K, d), torch.ones(1, device=DEV)
    want = {"hard": np.zeros(2, np.int64), "pmi": np.zeros(4, np.int64), "ldpc": np.zeros(3, np.int64), "twin": np.zeros(2, np.int64)}
    slack = 0
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        lead = np.ascontiguousarray(keys[::2 * R][delayed_groups(len(keys) // (2 * R), K, d)[0]])
        rho, scale = precoding_weights(snr, 0.0, R)
        counts, _, llr, pmi = p(ideal, est, _dev(keys), _dev(noise_sigma(snr)), _dev(rho), _dev(scale), one, want_llr=True)
        want["hard"] += counts.cpu().numpy().sum(axis=0)
        want["pmi"] += np.bincount(pmi.cpu().numpy().reshape(-1), minlength=4)
        want["ldpc"] += link_ldpc_host(code, lead, llr.cpu().numpy())[0].sum(axis=0)
        twin = link_precoded_host(link, keys, ideal.cpu().numpy(), est.cpu().numpy(), noise_sigma(snr), rho, scale, R, B, tau=derived_tau(R),
                                  pmi=pmi.cpu().numpy(), slots=K, delay=d)
        want["twin"] += twin[0].sum(axis=0)
        slack += int(twin[4].sum())
    assert hard.errors.cpu().tolist() == want["hard"].tolist() and ldpc.errors.cpu().tolist() == want["ldpc"].tolist()
    assert on_device.errors.cpu().tolist() == hard.errors.cpu().tolist()         # keys hashed on the device are the host's
    assert (np.abs(want["hard"] - want["twin"]) <= slack).all()
    for acc in (hard, ldpc, on_device):
        assert acc.pmi_histogram() == want["pmi"].tolist() and sum(acc.pmi_histogram()) == groups * 10
    print(f"2 x 2 precoded, B = {B}, d = {d}: BER {hard.result():.4f} against {instant.result():.4f} with instantaneous feedback (all "
          f"slots); LDPC BLER {ldpc.result():.3f}; applied-PMI histogram {hard.pmi_histogram()}; the twin's bit errors {int(want['twin'][0])} "
          f"against the device's {int(want['hard'][0])} with {slack} flagged decisions")
