"""``aft_link_soft_f32``, ``hip_ops.LinkSoftPlan``, ``linksim.RateAccumulator`` and ``evaluation.get_link_rates`` on the HIP device: the
kernel's LLRs and losses against the float64 definition through the two derived bounds below, their sign against the hard kernel, the
exact cases, independence of the batch, of the run and of the LLR output, operands in pinned memory, the 8- and 4-byte forms, no
unwritten element, the checked build, the sweep without a synchronisation, the entry point's refusals.

The shapes are tests/test_linksim_gpu.py's six (``GRIDS``: 120 x 14, odd 30 x 7, 128 x 40 with pilots 64 x 16, 2 x 1, 1 x 1, 3 x 5) and
a second frame with an odd number of elements, whose last pair holds one: 5 x 3.

The LLRs.  With u = 2^-24, every float32 operation within u of its result and no fast-math, in units of ``q = scale A (A p + 2 R)``
(linksim's docstring: A the outermost level, R the reach of a component of c; every exact ``|mu_k| <= A (A p + 2 R) = Q``):

* comp: the device's component of c errs by at most e_c R (tests/test_linksim_gpu.py derives e_c; its TAU is e_c), and ``|comp| <= R``.
* a_k = fl(fl(d) (2k - (L-1))): e_a = (1 + u)^2 - 1.   p = fma(E_re, E_re, E_im E_im), non-negative terms rounded twice: e_p = e_a.
* inner_k = fma(a_k, p, -2 comp), one rounding of the exact a_k' p' - 2 comp':  the perturbed operands give
  ((1 + e_a)(1 + e_p) - 1) |a_k| p + 2 e_c R, the rounding u times at most (1 + e_a)(1 + e_p) |a_k| p + 2 (1 + e_c) R:
  e_i = max((1 + e_a)(1 + e_p), 1 + e_c) (1 + u) - 1 (about 30 u) times (|a_k| p + 2 R).
* mu_k = fl(a_k inner_k):  e_mu = (1 + e_a)(1 + u)(1 + e_i) - 1 (about 33 u) times |a_k| (|a_k| p + 2 R) <= Q.
* a minimum of perturbed numbers is within the largest perturbation of the minimum: e_mu Q.
* Delta_j = fl(min1 - min0), both at most (1 + e_mu) Q in size:  e_D = 2 e_mu + 2 u (1 + e_mu) (about 68 u) times Q.
* Lambda_j = fl(scale Delta_j), scale the same float32 number on both sides:  e_lambda = e_D + u (2 + e_D) (about 70 u = 4.2e-6).

e_lambda <= TAU_CAP = 1e-5, at which tests/test_linksoft.py caps the width of the loss interval at 2e-2 of the loss.  (As there, a
product that underflows would escape the relative model: the channels are of order 1, and an estimate of exactly 0 makes every metric
an exact zero on the device and in the definition.)  Every LLR:  ``|llr_dev - llr_def| <= e_lambda q``.

The loss.  ``link_llrs_host(.., e_lambda)`` returns the exact interval [loss_lo, loss_hi] of the loss over all LLRs within e_lambda q.
What the device adds to a term ``softplus(z) = max(z, 0) + log1p(exp(-|z|))``, z = -+ fl(factor Lambda), relative to the term:

* the factor product moves z by u |z|; d softplus / dz = sigmoid(z) <= softplus(z) for z <= 0 and softplus(z) >= z for z > 0, so the
  term moves by at most exp(u |z|) - 1 of itself, with |z| <= 88 wherever exp(-|z|) is a normal number:  e_f = exp(88 u) - 1.
* exp to 3 ulp (6 u relative; log1p is less sensitive to its argument than proportionally), log1p to 2 ulp (4 u) -- the OpenCL limits
  the device library is built to --, the sum of the two non-negative parts rounds once:
  e_term = (1 + e_f)(1 + 6 u)(1 + 4 u)(1 + u) - 1 (about 99 u).
* the terms are non-negative, so a chain of n float32 additions is within (1 + u)^n - 1 of its sum: a thread adds the 2 m terms of each
  of its ceil(pairs / 256) element pairs, then 6 shuffle steps and the 3 additions across the four waves.
* the product with float32(1 / ln 2): the constant's rounding and the product's, 2 u.

e_s = (1 + e_term)(1 + u)^(2 m passes + 9 + 2) - 1, 1.0e-5 on the default grid at m = 8 and 1.6e-5 on 128 x 40.  A term whose exp(-|z|)
falls below float32's smallest normal 2^-126 is beyond any relative statement -- the definition keeps 1e-87 where float32 has no number
between 0 and 2^-149 -- and is below 2^-125 bit on both sides, so the comparison carries an absolute floor of 2^-100 per frame (more
than 2^-125 times the 2^16 bits of the largest frame here; 1e-30, against losses of order 1 to 1e4):

    loss_lo (1 - e_s) - floor <= loss_dev <= loss_hi (1 + e_s) + floor

The sign.  The nearest level has the smallest metric, so ``(llr_dev < 0) ^ sent``, summed per frame, is the hard kernel's bit-error
count except where the two kernels, which share the bits of c and p, decide a boundary differently: only at (element, axis) pairs
flagged at the hard kernel's TAU.  (Near a boundary the two metrics beside it are both about -a_k a_k+1 p, each within 2 u of itself,
and their exact difference is 4 d (comp - beta_b p): the soft decision can differ from the exact one on the device's c and p only
within about u |a_k a_k+1| p / d <= 14 u |beta_b| p of an outer boundary, inside TAU |beta_b| p; at the centre boundary, where
beta_b = 0 and the margin leaves nothing beyond e_c, the two metrics tie within u d p / 2 of comp = 0 and the tie reads as bit 0.  That
last sliver is not covered by the derivation, so there the assertion is a measured statement.)

The derived constants and how many frames had flags are printed; DESIGN.md records them."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib, ingest
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, make_pack, simulate_frames_host
from adafortitran_amd.hip_ops import LinkPlan, LinkSoftPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, LinkConfig, RateAccumulator, link_errors_host, link_llrs_host,
                                      llr_scale, noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator, lmmse_estimate_host
from test_chansim_gpu import _no_sync, _same_bits
from test_linksim import GRIDS, TAU_CAP, link_inputs
from test_linksim_gpu import TAU, U, _batch37, _dev, _pinned
from test_linksoft import sent_bits, soft_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -100
FACTORS = np.asarray(DEFAULT_FACTORS, dtype=np.float32)
ODD = "odd_elements_5x3"
SHAPES = (*GRIDS, ODD)


def derived_e_lambda() -> float:
    """The error of a device LLR in units of q; module docstring."""
    e_c = TAU
    e_a = e_p = (1 + U) ** 2 - 1
    e_i = max((1 + e_a) * (1 + e_p), 1 + e_c) * (1 + U) - 1
    e_mu = (1 + e_a) * (1 + U) * (1 + e_i) - 1
    e_d = 2 * e_mu + 2 * U * (1 + e_mu)
    return float(e_d + U * (2 + e_d))


def derived_e_s(cfg: LinkConfig) -> float:
    """The relative error the device adds to a frame's loss; module docstring."""
    e_f = np.expm1(88 * U)
    e_term = (1 + e_f) * (1 + 6 * U) * (1 + 4 * U) * (1 + U) - 1
    S, T = cfg.sim.ofdm
    passes = -(-((S * T + 1) // 2) // 256)
    return float((1 + e_term) * (1 + U) ** (2 * cfg.bits_per_symbol * passes + 9 + 2) - 1)


E_LAMBDA = derived_e_lambda()


def test_the_derived_bounds_are_below_the_cap():
    print(f"e_lambda = {E_LAMBDA:.3e} = {E_LAMBDA / U:.2f} u")
    for name in ("default_120x14", "pilot_bounds_128x40"):
        print(name, {m: f"e_s = {derived_e_s(LinkConfig(GRIDS[name][0], m)):.3e}" for m in BITS_PER_SYMBOL})
    assert 2 * TAU < E_LAMBDA <= 2 * TAU + 14 * U and E_LAMBDA <= TAU_CAP
    assert 99 * U < derived_e_s(LinkConfig(GRIDS["one_data_element_2x1"][0], 2)) < derived_e_s(LinkConfig(GRIDS["pilot_bounds_128x40"][0], 8)) < 2e-5


_odd = []


def _inputs(name):
    """``soft_inputs`` for the five shapes; for 5 x 3 the same recipe, two frames."""
    if name != ODD:
        return soft_inputs(name)
    if not _odd:
        sim = ChannelSimConfig(ofdm=(5, 3), pilot=(2, 1))
        ideal, pilots, meta = simulate_frames_host(sim, 3, np.arange(2))
        ideal = ideal.astype(np.complex64)
        est = {"lmmse": lmmse_estimate_host(sim, pilots.astype(np.complex64), meta).astype(np.complex64), "ideal": ideal}
        _odd.append((sim, frame_keys(3, np.arange(2)), noise_sigma(meta[:, 0]), llr_scale(meta[:, 0]), ideal, est))
    return _odd[0]


_plans, _wants = {}, {}


def _plan(name, m, cls=LinkSoftPlan):
    if (name, m, cls) not in _plans:
        _plans[name, m, cls] = cls(LinkConfig(_inputs(name)[0], m), DEV)
    return _plans[name, m, cls]


def _want(name, m, which):
    """The definition on an input set at the eight default factors, computed once: (loss, llr, loss_lo, loss_hi, q)."""
    if (name, m, which) not in _wants:
        sim, keys, sigma, scale, ideal, est = _inputs(name)
        _wants[name, m, which] = link_llrs_host(LinkConfig(sim, m), keys, ideal, est[which], sigma, scale, FACTORS, e_lambda=E_LAMBDA)
    return _wants[name, m, which]


def _poison_outputs(b, k, grid_m):
    """Leave free blocks of the sizes ``loss`` and ``llr`` will ask for filled with NaN, and check that the caching allocator hands
    them to the next requests of these sizes: an element the kernel leaves unwritten then shows."""
    junk = [torch.full(shape, float("nan"), device=DEV) for shape in ((b, k), (b, *grid_m))]
    del junk
    probe = [torch.empty(shape, device=DEV) for shape in ((b, k), (b, *grid_m))]
    assert all(p.isnan().all() for p in probe)
    del probe


def _check_loss(cfg, got: np.ndarray, want, columns=slice(None)):
    _, _, lo, hi, _ = want
    e_s = derived_e_s(cfg)
    assert got.shape == lo[:, columns].shape and np.isfinite(got).all()
    assert (lo[:, columns] * (1 - e_s) - FLOOR <= got).all() and (got <= hi[:, columns] * (1 + e_s) + FLOOR).all(), (got, lo, hi)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_kernel_against_the_float64_definition(m):
    worst_llr = worst_loss = 0.0
    for name in SHAPES:
        sim, keys, sigma, scale, ideal, est = _inputs(name)
        cfg, plan, b = LinkConfig(sim, m), _plan(name, m), len(keys)
        k, s, c, h, f = _dev(keys), _dev(sigma), _dev(scale), _dev(ideal), _dev(FACTORS)
        for which in est:
            want = _want(name, m, which)
            e = h if which == "ideal" else _dev(est[which])
            _poison_outputs(b, 8, (*sim.ofdm, m))
            loss8, llr = plan(h, e, k, s, c, f, want_llr=True)
            assert loss8.shape == (b, 8) and llr.shape == (b, *sim.ofdm, m) and loss8.dtype == llr.dtype == torch.float32 and llr.is_cuda
            got = llr.cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            err, q = np.abs(got - want[1]), want[4]
            assert (err <= E_LAMBDA * q).all(), (name, which, float((err / np.where(q > 0, q, 1)).max()))
            _check_loss(cfg, loss8.cpu().numpy().astype(np.float64), want)
            # without the LLR output, and at one factor with and without it: the same bits
            _poison_outputs(b, 8, (*sim.ofdm, m))
            bare8, none = plan(h, e, k, s, c, f)
            assert none is None
            loss1, llr1 = plan(h, e, k, s, c, f[:1], want_llr=True)
            bare1, _ = plan(h, e, k, s, c, f[:1])
            _same_bits([bare8, loss1, bare1, llr1], [loss8, loss8[:, :1], loss8[:, :1], llr])
            if q.any():
                worst_llr = max(worst_llr, float((err[q > 0] / q[q > 0]).max()))
            sizeable = want[0] > 1e-6
            if sizeable.any():
                worst_loss = max(worst_loss, float(np.abs(loss8.cpu().numpy()[sizeable] / want[0][sizeable] - 1).max()))
    print(f"m = {m}: largest |llr_dev - llr_def| / q = {worst_llr:.2e} (e_lambda = {E_LAMBDA:.2e}); "
          f"largest |loss_dev / loss_def - 1| = {worst_loss:.2e}")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_sign_of_the_llrs_against_the_hard_kernel(m):
    frames = with_flags = differing = 0
    for name in SHAPES:
        sim, keys, sigma, scale, ideal, est = _inputs(name)
        cfg = LinkConfig(sim, m)
        sent = torch.from_numpy(sent_bits(cfg, keys) == 1).to(DEV)
        mask = torch.from_numpy(cfg.data_mask).to(DEV)[None, :, :, None]
        k, s, c, h, f = _dev(keys), _dev(sigma), _dev(scale), _dev(ideal), _dev(FACTORS[:1])
        for which in est:
            e = h if which == "ideal" else _dev(est[which])
            _, llr = _plan(name, m)(h, e, k, s, c, f, want_llr=True)
            soft = (((llr < 0) ^ sent) & mask).sum(dim=(1, 2, 3)).cpu().numpy()
            hard = _plan(name, m, LinkPlan)(h, e, k, s)[:, 0].cpu().numpy()
            pairs = link_errors_host(cfg, keys, ideal, est[which], sigma, tau=TAU)[2].sum(axis=(1, 2, 3))
            assert (np.abs(soft - hard) <= pairs).all(), (name, which, soft, hard, pairs)
            frames += len(keys)
            with_flags += int((pairs > 0).sum())
            differing += int((soft != hard).sum())
    print(f"m = {m}: {with_flags} of {frames} frames had a flagged decision at tau = {TAU:.2e}; in {differing} the soft signs differ from the hard count")


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_exact_cases_through_the_entry_point_with_both_outputs_poisoned(m):
    """An estimate of exactly zero in frame 0: every metric is an exact zero, every LLR == 0 and every bit costs one bit.  Irregular
    pilot rows and columns: zeros exactly there.  Both outputs are filled with NaN first."""
    lib = _lib.load()
    sims = [(name, _inputs(name)[0]) for name in ("default_120x14", "odd_30x7", ODD, "one_data_element_2x1", "no_data_element_1x1",
                                                  "odd_last_alone_3x5")]
    sims.append(("pilot_lists", ChannelSimConfig(pilot=(4, 3), pilot_scs=(0, 7, 118, 119), pilot_symbols=(0, 1, 13))))
    for name, sim in sims:
        cfg = LinkConfig(sim, m)
        if name == "pilot_lists":
            ideal, _, meta = simulate_frames_host(sim, 3, np.arange(2))
            ideal, keys, sigma, scale = ideal.astype(np.complex64), frame_keys(3, np.arange(2)), noise_sigma(meta[:, 0]), llr_scale(meta[:, 0])
        else:
            _, keys, sigma, scale, ideal, _ = _inputs(name)
        b = len(keys)
        e = ideal.copy()
        e[0] = 0
        want = link_llrs_host(cfg, keys, ideal, e, sigma, scale, FACTORS, e_lambda=E_LAMBDA)
        loss = torch.full((b, 8), float("nan"), device=DEV)
        llr = torch.full((b, *sim.ofdm, m), float("nan"), device=DEV)
        ops = [_dev(a) for a in (ideal, e, keys, sigma, scale, FACTORS)]
        _lib.check(lib.aft_link_soft_f32(ctypes.byref(cfg.to_struct()), *(t.data_ptr() for t in ops), 8, loss.data_ptr(), llr.data_ptr(), b,
                                         _lib.current_stream_ptr(loss.device)), lib)
        got, got_loss = llr.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.isfinite(got_loss).all()                    # no element is left unwritten
        assert (got[0] == 0).all() and (got[:, ~cfg.data_mask] == 0).all()
        assert (np.abs(got - want[1]) <= E_LAMBDA * want[4]).all()
        assert (np.abs(got_loss[0] - m * cfg.data_elements) <= derived_e_s(cfg) * m * cfg.data_elements).all()
        _check_loss(cfg, got_loss, want)
        if name == "pilot_lists":
            assert (~cfg.data_mask).sum() == 12 and (got[1][cfg.data_mask] != 0).all()
        if name == "odd_last_alone_3x5":           # element 14, alone in the last pair: written, and not with a pilot's zeros
            assert cfg.data_mask[2, 4] and (got[1, 2, 4] != 0).all()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_a_frame_does_not_depend_on_its_batch_its_position_or_the_run(m):
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, scale, ideal, est = _inputs(name)
        plan = _plan(name, m)
        alone = plan(_dev(ideal[:1]), _dev(est["lmmse"][:1]), _dev(keys[:1]), _dev(sigma[:1]), _dev(scale[:1]), f, want_llr=True)
        h, e, k, s = (_dev(a) for a in _batch37(name))
        c = (1.0 / s.double() ** 2).float()
        batch = plan(h, e, k, s, c, f, want_llr=True)
        for out, one in zip(batch, alone):
            _same_bits([out[4:5], out[36:37]], [one, one])
        for i in (0, 17, 35):
            _same_bits(plan(h[i:i + 1], e[i:i + 1], k[i:i + 1], s[i:i + 1], c[i:i + 1], f, want_llr=True), [batch[0][i:i + 1], batch[1][i:i + 1]])
        _same_bits(plan(h, e, k, s, c, f, want_llr=True), batch)                     # a second run of the same batch
    sim, keys, sigma, scale, ideal, est = _inputs(ODD)                               # an odd frame: every second one starts mid-pair
    plan = _plan(ODD, m)
    both = plan(_dev(ideal), _dev(est["lmmse"]), _dev(keys), _dev(sigma), _dev(scale), f, want_llr=True)
    second = plan(_dev(ideal[1:]), _dev(est["lmmse"][1:]), _dev(keys[1:]), _dev(sigma[1:]), _dev(scale[1:]), f, want_llr=True)
    _same_bits(second, [both[0][1:], both[1][1:]])


def test_operands_in_pinned_memory_and_what_the_plan_refuses():
    for name in ("default_120x14", "odd_30x7"):
        plan = _plan(name, 4)
        h, e, k, s = _batch37(name)
        c = (1.0 / s.astype(np.float64) ** 2).astype(np.float32)
        want = plan(_dev(h), _dev(e), _dev(k), _dev(s), _dev(c), _dev(FACTORS), want_llr=True)
        got = plan(_dev(h), _dev(e), _pinned(k), _pinned(s).reshape(-1, 1), _pinned(c), _pinned(FACTORS), want_llr=True)   # read in place
        _same_bits(got, want)
    hd, ed, kd, sd, cd, fd = _dev(h), _dev(e), _dev(k), _dev(s), _dev(c), _dev(FACTORS)
    for args, word in (((hd, ed, torch.from_numpy(np.array(k).view(np.int64)), sd, cd, fd), "pinned host memory"),
                       ((hd, ed, kd, sd, torch.from_numpy(np.array(c)), fd), "pinned host memory"),
                       ((hd, ed, kd, sd, cd, torch.from_numpy(np.array(FACTORS))), "pinned host memory"),
                       ((hd, ed, kd[:5], sd, cd, fd), "one value per frame"), ((hd, ed, kd, sd[:5], cd, fd), "one value per frame"),
                       ((hd, ed, kd, sd, cd[:5], fd), "one value per frame"),
                       ((hd, ed, kd.to(torch.int32), sd, cd, fd), "keys must be torch.int64"), ((hd, ed, kd, sd.double(), cd, fd), "sigma must be torch.float32"),
                       ((hd, ed, kd, sd, cd.double(), fd), "scale must be torch.float32"), ((hd, ed, kd, sd, cd, fd.double()), "factors must be torch.float32"),
                       ((hd, ed, kd, sd, cd, fd[:0]), "between 1 and 8"), ((hd, ed, kd, sd, cd, torch.ones(9, device=DEV)), "between 1 and 8"),
                       ((hd, ed, kd, sd, cd, (1.0,)), "between 1 and 8"),
                       ((hd.to(torch.complex128), ed, kd, sd, cd, fd), "ideal must be complex64"), ((hd, ed[:5], kd, sd, cd, fd), "ideal's shape"),
                       ((hd[:, :, :3], ed, kd, sd, cd, fd), "Expected ideal shape"), ((hd[:0], ed[:0], kd[:0], sd[:0], cd[:0], fd), "Expected ideal shape"),
                       ((hd.cpu(), ed, kd, sd, cd, fd), "must live on")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    with pytest.raises(ValueError, match="LinkSoftPlan runs on a HIP device"):
        LinkSoftPlan(LinkConfig(), "cpu")
    with pytest.raises(ValueError, match="LinkSoftPlan needs a linksim.LinkConfig"):
        LinkSoftPlan(ChannelSimConfig(), DEV)


@pytest.mark.parametrize("m", (2, 6, 8))
def test_the_8_and_4_byte_forms_on_bases_off_16_bytes(m):
    """The caching allocator only hands out 512-byte aligned blocks; bases 8 and 4 bytes off go through the entry point directly."""
    plan = _plan("default_120x14", m)
    h, e, k, s = (_dev(a) for a in _batch37("default_120x14"))
    c, f = (1.0 / s.double() ** 2).float(), _dev(FACTORS)
    want_loss, want_llr = plan(h, e, k, s, c, f, want_llr=True)
    n = h.numel()
    fh, fe = (torch.empty(n + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
    fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
    assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
    lib = _lib.load()
    for hp, ep, off in ((fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (h.data_ptr(), fe.data_ptr() + 8, 0), (h.data_ptr(), e.data_ptr(), 8),
                        (h.data_ptr(), e.data_ptr(), 4), (fh.data_ptr() + 8, fe.data_ptr() + 8, 12)):
        loss = torch.full((37, 8), float("nan"), device=DEV)
        llr = torch.full((want_llr.numel() + 4,), float("nan"), device=DEV)
        _lib.check(lib.aft_link_soft_f32(ctypes.byref(plan.link), hp, ep, k.data_ptr(), s.data_ptr(), c.data_ptr(), f.data_ptr(), 8,
                                         loss.data_ptr(), llr.data_ptr() + off, 37, _lib.current_stream_ptr(loss.device)), lib)
        at = off // 4
        _same_bits([loss, llr[at:at + want_llr.numel()]], [want_loss, want_llr.reshape(-1)])
        assert llr[:at].isnan().all() and llr[at + want_llr.numel():].isnan().all()      # nothing beside the output is written


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_soft_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_soft_f32")
    for name in SHAPES:
        sim, keys, sigma, scale, ideal, est = _inputs(name)
        for m in BITS_PER_SYMBOL:
            args = (_dev(ideal), _dev(est["lmmse"]), _dev(keys), _dev(sigma), _dev(scale), _dev(FACTORS))
            _same_bits(_plan(name, m)(*args, want_llr=True, lib=lib), _plan(name, m)(*args, want_llr=True))


@pytest.mark.parametrize("m", (2, 6))
def test_rate_accumulator_runs_from_the_loader_without_a_synchronisation(m):
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, m)
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 5, device=DEV, seed=2)
    with_est, perfect, on_device = (RateAccumulator(cfg, DEV, seed=2, factors=DEFAULT_FACTORS) for _ in range(3))
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
    assert len(seen) == 5 and with_est.frames == perfect.frames == 80 and with_est.loss.is_cuda and with_est.loss.dtype == torch.float64
    # keys hashed with torch ops on the device are the host's; sigma and scale are float32 roundings of a double power formed there
    torch.testing.assert_close(on_device.loss, with_est.loss, rtol=1e-5, atol=0)
    lo, hi = np.zeros((2, 8)), np.zeros((2, 8))
    for ideal, est, meta in seen:
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        snr, h = meta[1].numpy().reshape(-1), ideal.cpu().numpy()
        for i, e in enumerate((est.cpu().numpy(), h)):
            want = link_llrs_host(cfg, frame_keys(2, g), h, e, noise_sigma(snr), llr_scale(snr), FACTORS, e_lambda=E_LAMBDA)
            lo[i] += want[2].sum(axis=0)
            hi[i] += want[3].sum(axis=0)
    e_s = derived_e_s(cfg)
    got = np.stack([with_est.loss.cpu().numpy(), perfect.loss.cpu().numpy()])
    print(f"m = {m}: loss with the LMMSE estimate {got[0].round(1).tolist()}, with the channel {got[1].round(1).tolist()}; "
          f"interval widths {((hi - lo) / hi).max():.2e}")
    assert (lo * (1 - e_s) - 80 * FLOOR <= got).all() and (got <= hi * (1 + e_s) + 80 * FLOOR).all()
    elements = 80 * cfg.data_elements
    for acc, i in ((with_est, 0), (perfect, 1)):
        rates = np.asarray(acc.result())
        assert (m - hi[i] * (1 + e_s) / elements - 1e-12 <= rates).all() and (rates <= m - lo[i] * (1 - e_s) / elements + 1e-12).all()
        assert acc.result_gmi() == rates.max()
    assert perfect.result_gmi() >= with_est.result_gmi()


def test_rate_sweep_over_simulated_packs():
    from adafortitran_amd.evaluation import get_link_rates
    sim = ChannelSimConfig()
    cfg = LinkConfig(sim, 6)
    model = LmmseEstimator(sim).to(DEV)
    packs = {snr: make_pack(sim, 128, seed=20 + snr, snr_db=snr) for snr in (0, 10, 20)}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, sim.pilot, 64, device=DEV, shuffle=False)) for snr, pack in packs.items()]
    lmmse, perfect = get_link_rates(model, loaders, cfg, seed=1), get_link_rates(None, loaders, cfg, seed=1)
    print("rate in bit/symbol with the LMMSE estimate", lmmse, " with the channel", perfect)
    assert list(lmmse) == list(perfect) == [0, 10, 20]
    assert 0 < perfect[0] < perfect[10] < perfect[20] <= 6
    assert all(perfect[snr] >= lmmse[snr] for snr in packs)


def test_every_refusal_of_the_entry_point_launches_nothing():
    sim, keys, sigma, scale, ideal, est = _inputs("default_120x14")
    lib, b = _lib.load(), len(keys)
    cfg = LinkConfig(sim, 4)
    loss = torch.full((b, 8), float("nan"), device=DEV)
    llr = torch.full((b, *sim.ofdm, 4), float("nan"), device=DEV)
    h, e, k, s, c, f = _dev(ideal), _dev(est["lmmse"]), _dev(keys), _dev(sigma), _dev(scale), _dev(FACTORS)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), scale=c.data_ptr(), factors=f.data_ptr(),
                n_factors=8, loss=loss.data_ptr(), llr=llr.data_ptr(), batch=b)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.to_struct() if p is None else p
        return lib.aft_link_soft_f32(ctypes.byref(p), *(a[n] for n in good), None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_soft_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for name in ("ideal", "est", "keys", "sigma", "scale", "factors", "loss"):
        refused(E, "NULL pointer", **{name: None})
    for name in ("ideal", "est", "keys"):
        refused(E, "8-byte", **{name: good[name] + 4})
    for name in ("sigma", "scale", "factors", "loss", "llr"):
        refused(E, "4-byte", **{name: good[name] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for n in (0, 9, -1):
        refused(E, f"n_factors = {n} is outside 1..8", n_factors=n)

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
    assert loss.isnan().all() and llr.isnan().all()                                  # nothing was launched
    assert call() == _abi.AFT_OK and call(llr=None, loss=loss.data_ptr()) == _abi.AFT_OK      # a NULL llr is legal
    torch.cuda.synchronize()
    _same_bits([loss, llr], _plan("default_120x14", 4)(h, e, k, s, c, f, want_llr=True))     # ... and the good call writes it all
    # a grid whose every element is a pilot is legal: loss 0, LLR 0
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), 8).to_struct()
    assert call(one, batch=1) == _abi.AFT_OK and loss[0].tolist() == [0.0] * 8 and llr.reshape(-1)[:8].tolist() == [0.0] * 8
