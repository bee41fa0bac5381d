"""``aft_link_errors_f32``, ``hip_ops.LinkPlan``, ``linksim.LinkAccumulator`` and ``evaluation.get_link_stats`` on the HIP device: the
kernel's counts against the float64 definition through the margin rule below, the exact cases, independence of the batch and of the
run, pinned keys and noise scales, the 8-byte load form, no unwritten count, the checked build, the sweep without a synchronisation,
the entry point's refusals.

The shapes (tests/test_linksim.py ``GRIDS``; estimates from ``lmmse_estimate_host`` and from the channel itself; m = 2, 4, 6, 8):

    default 120 x 14, pilots 12 x 2, 3 frames     the default path: 16-byte loads, 840 pairs over 256 threads
    30 x 7, pilots 5 x 3, 5 frames                odd T: 8-byte loads, a ragged last pass
    128 x 40, pilots 64 x 16, 2 frames            many elements per thread, the pilot lists at their bounds
    2 x 1, pilot 1 x 1, 1 frame                   one data element
    1 x 1, pilot 1 x 1, 1 frame                   no data element: counts (0, 0)
    3 x 5, pilot 1 x 1 at (1, 2), 2 frames        an odd number of elements whose last is data: alone in the last pair

The comparison rule.  A hard decision is a comparison ``comp >= beta_b p``; the device evaluates both sides in float32, so where the two
sides are closer than its rounding error the decision may fall either way, and nowhere else.  The definition returns, per (element,
axis, boundary), the margin ``|comp - beta_b p| / ((|H||x| + |noise|) |E| + |beta_b| p)``; an (element, axis) is flagged when a boundary
has margin <= tau.  If the device's comp errs by at most e_c (|H||x| + |noise|) |E| and its beta_b p by at most e_t |beta_b| p, every
unflagged decision is the definition's for tau = max(e_c, e_t).  u = 2^-24 is float32's unit roundoff and every float32 operation errs
by at most u times its result; sincospi errs by at most 4 ulp, log and sqrt by 3 ulp each (the OpenCL full-profile limits the device
library is built to; an ulp is at most 2 u relative, and at most 2 u in absolute terms for a sine or cosine); the build has no
fast-math.  Writing Y = |H||x| + |noise|, per real component (``derived_tau``):

* x: d is rounded to float32 once and multiplied by a small integer: |dx| <= ((1+u)^2 - 1) |x| = e_x |x|.
* H x: one product and one fused multiply-add per component; the perturbed x gives e_x |H||x|, the two roundings 2 u |H||x|:
  e_h = (1 + e_x)(1 + u)^2 - 1 (about 4 u) times |H||x|.
* noise: u1 and u2 are exact in float32, the doubling and the reduction of the angle are exact.  -ln u1 to 6 u relative, its root halves
  that (3 u) and adds its own 6 u, the product with sigma (the same float32 number on both sides) rounds once: the radius is within
  e_r = (1 + 3 u)(1 + 6 u)(1 + u) - 1 (about 10 u); a component of exp(j 2 pi u2) is within 8 u; their product, formed inside the fused
  multiply-add, within e_n = e_r + 8 u (1 + e_r) (about 18 u) times |noise|.
* y = fma(radius, component, H x): its rounding is u Y (1 + e_n):  e_y = max(e_h, e_n) + u (1 + e_n) (about 19 u) times Y.
* c = y conj(E): a product and a fused multiply-add per component.  The perturbed y gives e_y Y (|E_re| + |E_im|) <= sqrt(2) e_y Y |E|,
  the two roundings 2 u |y||E| <= 2 u (1 + e_y) Y |E|:  e_c = sqrt(2) e_y + 2 u (1 + e_y) (about 29 u).
* beta_b p: p = fma(E_re, E_re, E_im E_im) is a sum of non-negative terms rounded twice, 2 d is float32's rounding of the exact value,
  the product with p rounds, the product with the integer b - L/2 rounds:  e_t = (1 + u)^5 - 1 (about 5 u).

tau = max(e_c, e_t) = 1.72e-6, below the 1e-5 at which tests/test_linksim.py caps the flagged share at 1e-3.  (A float32 product that
underflows would escape the relative model; the channels here are of order 1, and an estimate of exactly 0 makes both sides exact
zeros on the device and in the definition.)  Per frame:

    |bit errors - definition's|    <= the (element, axis) pairs flagged in that frame   (the Gray map: one boundary, one bit)
    |symbol errors - definition's| <= the elements flagged in that frame
    both equal the definition's in every frame with nothing flagged

How many frames had flags is printed; DESIGN.md records it."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, make_pack, simulate_frames_host
from adafortitran_amd.hip_ops import LinkPlan
from adafortitran_amd.linksim import BITS_PER_SYMBOL, LinkAccumulator, LinkConfig, link_errors_host, noise_sigma
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linksim import GRIDS, SHARE_CAP, TAU_CAP, flagged_share, link_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
POISON = -7777                 # no count is negative


def derived_tau() -> float:
    """The relative error the device's two sides of a decision can carry; module docstring."""
    e_x = (1 + U) ** 2 - 1
    e_h = (1 + e_x) * (1 + U) ** 2 - 1
    e_r = (1 + 3 * U) * (1 + 6 * U) * (1 + U) - 1
    e_n = e_r + 8 * U * (1 + e_r)
    e_y = max(e_h, e_n) + U * (1 + e_n)
    e_c = np.sqrt(2.0) * e_y + 2 * U * (1 + e_y)
    e_t = (1 + U) ** 5 - 1
    return float(max(e_c, e_t))


TAU = derived_tau()


def test_the_derived_tau_is_below_the_cap():
    print(f"tau = {TAU:.3e} = {TAU / U:.2f} u")
    assert 28 * U < TAU <= 30 * U and TAU <= TAU_CAP


def _dev(a: np.ndarray) -> torch.Tensor:
    a = np.array(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def _pinned(a: np.ndarray) -> torch.Tensor:
    a = np.array(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).pin_memory()


def _poison_counts(b):
    """Leave a free block of the size ``counts`` will ask for filled with an impossible count, and check that the caching allocator
    hands that block to the next request of this size: an entry the kernel leaves unwritten then shows."""
    junk = torch.full((b, 2), POISON, dtype=torch.int32, device=DEV)
    del junk
    probe = torch.empty((b, 2), dtype=torch.int32, device=DEV)
    assert (probe == POISON).all()
    del probe


_plans, _wants = {}, {}


def _plan(name, m):
    if (name, m) not in _plans:
        _plans[name, m] = LinkPlan(LinkConfig(GRIDS[name][0], m), DEV)
    return _plans[name, m]


def _want(name, m, which):
    """The definition's (counts, flagged pairs per frame, flagged elements per frame, flagged share), computed once."""
    if (name, m, which) not in _wants:
        sim, keys, sigma, ideal, est = link_inputs(name)
        cfg = LinkConfig(sim, m)
        counts, _, flags = link_errors_host(cfg, keys, ideal, est[which], sigma, tau=TAU)
        _wants[name, m, which] = (counts, flags.sum(axis=(1, 2, 3)), flags.any(axis=3).sum(axis=(1, 2)), flagged_share(cfg, flags))
    return _wants[name, m, which]


def _check_against(got: np.ndarray, want):
    counts, pairs, elems, _ = want
    assert got.shape == counts.shape and (got >= 0).all()
    assert (np.abs(got[:, 0] - counts[:, 0]) <= pairs).all(), (got, counts, pairs)
    assert (np.abs(got[:, 1] - counts[:, 1]) <= elems).all(), (got, counts, elems)
    clean = pairs == 0
    assert (got[clean] == counts[clean]).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    frames = with_flags = differing = 0
    for name in GRIDS:
        sim, keys, sigma, ideal, est = link_inputs(name)
        plan = _plan(name, m)
        k, s, h = _dev(keys), _dev(sigma), _dev(ideal)
        for which in est:
            want = _want(name, m, which)
            e = h if which == "ideal" else _dev(est[which])
            _poison_counts(len(keys))
            counts = plan(h, e, k, s)
            assert counts.shape == (len(keys), 2) and counts.dtype == torch.int32 and counts.is_cuda
            got = counts.cpu().numpy().astype(np.int64)
            assert want[3] <= SHARE_CAP
            _check_against(got, want)
            frames += len(keys)
            with_flags += int((want[1] > 0).sum())
            differing += int((got != want[0]).any(axis=1).sum())
    sim, keys, sigma, ideal, est = link_inputs("no_data_element_1x1")
    assert _plan("no_data_element_1x1", m)(_dev(ideal), _dev(ideal), _dev(keys), _dev(sigma)).tolist() == [[0, 0]]
    print(f"m = {m}: {with_flags} of {frames} frames had a flagged decision at tau = {TAU:.2e}; {differing} differ from the definition")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_exact_cases(m):
    for name in ("default_120x14", "odd_30x7", "pilot_bounds_128x40", "one_data_element_2x1", "odd_last_alone_3x5"):
        sim, keys, sigma, ideal, _ = link_inputs(name)
        cfg, plan, b = LinkConfig(sim, m), _plan(name, m), len(keys)
        k, h, zero = _dev(keys), _dev(ideal), torch.zeros(b, device=DEV)
        _poison_counts(b)
        assert not plan(h, h, k, zero).any()                                     # the estimate is the channel, no noise: no error
        if name == "odd_last_alone_3x5":           # min |H| is 0.549: the MSB of each axis flips at every m; (26, 13) without element 14
            assert plan(h, -h, k, zero).tolist() == [[28, 14]] * 2
        if m == 2:                                                               # the estimate points the other way: every bit flips
            assert plan(h, -h, k, zero).tolist() == [[2 * cfg.data_elements, cfg.data_elements]] * b
        # an estimate of exactly zero: both sides of every comparison are exact zeros, on the device and in the definition
        e = ideal.copy()
        e[0] = 0
        want = link_errors_host(cfg, keys[:1], ideal[:1], e[:1], sigma[:1])
        got = plan(h, _dev(e), k, _dev(sigma))[:1].cpu().numpy()
        assert np.isfinite(got).all() and (got == want).all() and (cfg.data_elements < 10 or want[0, 1] > 0)


_many = {}


def _batch37(name):
    """37 frames of seed 12 with LS-interpolated estimates; frames 4 and 36 are frame 0 of ``link_inputs`` with its LMMSE estimate."""
    if name not in _many:
        sim, keys, sigma, ideal, est = link_inputs(name)
        h, pil, meta = simulate_frames_host(sim, 12, np.arange(37))
        h, e = h.astype(np.complex64), ls_interpolate(sim, pil.astype(np.complex64))
        k, s = frame_keys(12, np.arange(37)), noise_sigma(meta[:, 0])
        for i in (4, 36):
            h[i], e[i], k[i], s[i] = ideal[0], est["lmmse"][0], keys[0], sigma[0]
        _many[name] = (h, e, k, s)
    return _many[name]


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_frame_does_not_depend_on_its_batch_its_position_or_the_run(m):
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, ideal, est = link_inputs(name)
        plan = _plan(name, m)
        alone = plan(_dev(ideal[:1]), _dev(est["lmmse"][:1]), _dev(keys[:1]), _dev(sigma[:1]))
        h, e, k, s = (_dev(a) for a in _batch37(name))
        batch = plan(h, e, k, s)
        _same_bits([batch[4:5], batch[36:37]], [alone, alone])
        one_by_one = torch.cat([plan(h[i:i + 1], e[i:i + 1], k[i:i + 1], s[i:i + 1]) for i in (0, 17, 35)])
        _same_bits([batch[[0, 17, 35]]], [one_by_one])
        _same_bits([plan(h, e, k, s)], [batch])                                  # a second run of the same batch


def test_keys_and_sigma_in_pinned_memory_and_what_the_plan_refuses():
    for name in ("default_120x14", "odd_30x7"):
        plan = _plan(name, 4)
        h, e, k, s = _batch37(name)
        want = plan(_dev(h), _dev(e), _dev(k), _dev(s))
        got = plan(_dev(h), _dev(e), _pinned(k), _pinned(s).reshape(-1, 1))          # read in place; any shape of 37 values
        _same_bits([got], [want])
    hd, ed, kd, sd = _dev(h), _dev(e), _dev(k), _dev(s)
    for args, word in (((hd, ed, torch.from_numpy(np.array(k).view(np.int64)), sd), "pinned host memory"),
                       ((hd, ed, kd, torch.from_numpy(np.array(s))), "pinned host memory"),
                       ((hd, ed, kd[:5], sd), "one value per frame"), ((hd, ed, kd, sd[:5]), "one value per frame"),
                       ((hd, ed, kd.to(torch.int32), sd), "keys must be torch.int64"), ((hd, ed, kd, sd.double()), "sigma must be torch.float32"),
                       ((hd.to(torch.complex128), ed, kd, sd), "ideal must be complex64"), ((hd, ed[:5], kd, sd), "ideal's shape"),
                       ((hd[:, :, :3], ed, kd, sd), "Expected ideal shape"), ((hd[:0], ed[:0], kd[:0], sd[:0]), "Expected ideal shape"),
                       ((hd.cpu(), ed, kd, sd), "must live on")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    with pytest.raises(ValueError, match="HIP device"):
        LinkPlan(LinkConfig(), "cpu")
    with pytest.raises(ValueError, match="LinkConfig"):
        LinkPlan(ChannelSimConfig(), DEV)


@pytest.mark.parametrize("m", (2, 8))
def test_the_8_byte_load_form_on_bases_off_16_bytes(m):
    """The caching allocator only hands out 512-byte aligned blocks; bases 8 bytes off go through the entry point directly."""
    plan = _plan("default_120x14", m)
    h, e, k, s = (_dev(a) for a in _batch37("default_120x14"))
    want = plan(h, e, k, s)
    n = h.numel()
    fh, fe = (torch.empty(n + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
    fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
    assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
    counts = torch.full((37, 2), POISON, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().aft_link_errors_f32(ctypes.byref(plan.link), fh.data_ptr() + 8, fe.data_ptr() + 8, k.data_ptr(),
                                               s.data_ptr(), counts.data_ptr(), 37, _lib.current_stream_ptr(counts.device)))
    _same_bits([counts], [want])
    # ... and with one base only off: still the 8-byte form
    counts.fill_(POISON)
    _lib.check(_lib.load().aft_link_errors_f32(ctypes.byref(plan.link), h.data_ptr(), fe.data_ptr() + 8, k.data_ptr(),
                                               s.data_ptr(), counts.data_ptr(), 37, _lib.current_stream_ptr(counts.device)))
    _same_bits([counts], [want])


def test_checked_build_gives_the_same_counts():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_errors_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_errors_f32")
    for name in GRIDS:
        sim, keys, sigma, ideal, est = link_inputs(name)
        for m in BITS_PER_SYMBOL:
            args = (_dev(ideal), _dev(est["lmmse"]), _dev(keys), _dev(sigma))
            _same_bits([_plan(name, m)(*args, lib=lib)], [_plan(name, m)(*args)])


@pytest.mark.parametrize("m", (2, 6))
def test_accumulator_runs_from_the_loader_without_a_synchronisation(m):
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, m)
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 5, device=DEV, seed=2)
    with_est, perfect, on_device = (LinkAccumulator(cfg, DEV, seed=2) for _ in range(3))
    it = iter(loader)
    first = next(it)
    seen = []

    def step(batch):
        pil, ideal, meta = batch
        est = model(pil, meta)
        with_est.update(est, ideal, meta)
        perfect.update(None, ideal, meta)
        on_device.update(est, ideal, frame_ids=meta[0].to(DEV, non_blocking=True), snr_db=meta[1].to(DEV, non_blocking=True))
        seen.append((ideal, est, meta))

    step(first)                                   # the first batch builds the plans and the pinned blocks: outside the guard
    torch.cuda.synchronize()
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                          # the mode is honoured: what follows is not vacuous
        for batch in it:
            step(batch)
    assert len(seen) == 5 and with_est.frames == perfect.frames == 80 and with_est.errors.is_cuda and with_est.errors.dtype == torch.int64
    _same_bits([on_device.errors], [with_est.errors])              # keys hashed with torch ops on the device: the host's keys
    want = np.zeros((2, 2), dtype=np.int64)
    slack = np.zeros((2, 2), dtype=np.int64)
    for ideal, est, meta in seen:
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        keys, sigma, h = frame_keys(2, g), noise_sigma(meta[1].numpy().reshape(-1)), ideal.cpu().numpy()
        for i, e in enumerate((est.cpu().numpy(), h)):
            counts, _, flags = link_errors_host(cfg, keys, h, e, sigma, tau=TAU)
            assert flagged_share(cfg, flags) <= SHARE_CAP
            want[i] += counts.sum(axis=0)
            slack[i] += [flags.sum(), flags.any(axis=3).sum()]
    got = np.stack([with_est.errors.cpu().numpy(), perfect.errors.cpu().numpy()])
    print(f"m = {m}: errors (bit, symbol) with the LMMSE estimate {got[0].tolist()}, with the channel {got[1].tolist()}; "
          f"definition {want.tolist()}; flagged {slack.tolist()}")
    assert (np.abs(got - want) <= slack).all()
    assert abs(with_est.result() - want[0, 0] / (80 * cfg.bits_per_frame)) <= slack[0, 0] / (80 * cfg.bits_per_frame)
    assert abs(perfect.result_ser() - want[1, 1] / (80 * cfg.data_elements)) <= slack[1, 1] / (80 * cfg.data_elements)
    assert perfect.result() < with_est.result()


def test_link_sweep_over_simulated_packs():
    from adafortitran_amd.evaluation import get_link_stats
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 4)
    model = LmmseEstimator(sim).to(DEV)
    packs = {snr: make_pack(sim, 256, seed=20 + snr, snr_db=snr) for snr in (0, 10, 20)}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, sim.pilot, 128, device=DEV, shuffle=False)) for snr, pack in packs.items()]
    lmmse, perfect = get_link_stats(model, loaders, cfg, seed=1), get_link_stats(None, loaders, cfg, seed=1)
    print("BER with the LMMSE estimate", lmmse, " with the channel", perfect)
    assert list(lmmse) == list(perfect) == [0, 10, 20]
    assert lmmse[0] > lmmse[10] > lmmse[20] > 0 and perfect[0] > perfect[10] > perfect[20] > 0
    assert all(perfect[snr] < lmmse[snr] for snr in packs)


def test_every_refusal_of_the_entry_point_launches_nothing():
    sim, keys, sigma, ideal, est = link_inputs("default_120x14")
    lib, b = _lib.load(), len(keys)
    cfg = LinkConfig(sim, 4)
    counts = torch.full((b, 2), POISON, dtype=torch.int32, device=DEV)
    h, e, k, s = _dev(ideal), _dev(est["lmmse"]), _dev(keys), _dev(sigma)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), counts=counts.data_ptr(), batch=b)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return lib.aft_link_errors_f32(ctypes.byref(p), a["ideal"], a["est"], a["keys"], a["sigma"], a["counts"], a["batch"], None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_link_errors_f32(None, good["ideal"], good["est"], good["keys"], good["sigma"], good["counts"], b, None)
    assert rc == E and "NULL pointer" in lib.aft_last_error().decode()
    for name in ("ideal", "est", "keys", "sigma", "counts"):
        refused(E, "NULL pointer", **{name: None})
    for name in ("ideal", "est", "keys"):
        refused(E, "8-byte", **{name: good[name] + 4})
    for name in ("sigma", "counts"):
        refused(E, "4-byte", **{name: good[name] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)

    def struct(**fields):
        p = cfg.to_struct()
        for name, value in fields.items():
            if isinstance(value, tuple):
                getattr(p, name)[value[0]] = value[1]
            else:
                setattr(p, name, value)
        return p

    for fields, word in ((dict(num_scs=0), "num_scs = 0"), (dict(num_symbols=-1), "num_symbols = -1"),
                         (dict(num_scs=1 << 16, num_symbols=(1 << 15) + 1), "more than 2^31 elements"),
                         (dict(pilot_scs=65), "pilot_scs = 65 is outside 1..64"), (dict(pilot_scs=0), "pilot_scs = 0"),
                         (dict(pilot_symbols=17), "pilot_symbols = 17 is outside 1..16"), (dict(pilot_symbols=0), "pilot_symbols = 0"),
                         (dict(num_symbols=1), "larger than the ofdm grid"), (dict(num_scs=11), "larger than the ofdm grid"),
                         (dict(pilot_sc_index=(1, 5)), "pilot_sc_index[1] = 5"), (dict(pilot_sc_index=(3, 15)), "pilot_sc_index[3] = 15"),
                         (dict(pilot_sc_index=(0, -1)), "pilot_sc_index[0] = -1"), (dict(pilot_sc_index=(11, 120)), "pilot_sc_index[11] = 120"),
                         (dict(pilot_symbol_index=(1, 14)), "pilot_symbol_index[1] = 14"), (dict(pilot_symbol_index=(1, 3)), "strictly increasing"),
                         (dict(bits_per_symbol=0), "bits_per_symbol = 0"), (dict(bits_per_symbol=3), "bits_per_symbol = 3"),
                         (dict(bits_per_symbol=10), "bits_per_symbol = 10"), (dict(bits_per_symbol=-2), "bits_per_symbol = -2")):
        refused(SH, word, p=struct(**fields))
    torch.cuda.synchronize()
    assert (counts == POISON).all()                                                  # nothing was launched
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    _same_bits([counts], [_plan("default_120x14", 4)(h, e, k, s)])                   # ... and the good call writes it all
    # a grid whose every element is a pilot is legal
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), 8).to_struct()
    assert call(one, batch=1) == _abi.AFT_OK and counts[0].tolist() == [0, 0]
