"""What tests/test_linksm_gpu.py and tests/test_linkjoint_gpu.py share: the two-stream link's plans, operands and runs on the HIP device by
detector name (``"zf"`` / ``"mmse"``: ``aft_link_sm_f32`` through ``LinkSmPlan``; ``"joint"``: ``aft_link_joint_f32`` through
``LinkJointPlan``, which has no ``reg``), and the bodies of the tests that ask both entry points the same thing: independence of the
batch, of the position and of the run, no unwritten element and the 8- and 4-byte forms, the checked build, the refusals of the plan and
of the entry point, and the coded accumulators.  Each file calls a body under its own test name with the detectors it runs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkJointPlan, LinkSmPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, DEFAULT_FACTORS, JOINT_DETECTOR, BlockErrorAccumulator, CodeConfig,
                                      LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig, link_decode_host, link_ldpc_host, noise_sigma,
                                      sm_weights)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync, _same_bits
from test_linkmrc import MRC_ODD
from test_linksim_gpu import _dev
from test_linksm import sm_inputs

DEV = "cuda"
POISON = -7777
FACTORS = np.asarray(DEFAULT_FACTORS[:3], dtype=np.float32)
_plans, _ops = {}, {}


def plan_class(detector):
    return LinkJointPlan if detector == JOINT_DETECTOR else LinkSmPlan


def weights(snr, R, detector):
    """The per-frame and per-group operands after ``sigma``, in the entry point's order: ``(rho, scale)`` and, for a linear detector, ``reg``."""
    if detector == JOINT_DETECTOR:
        return sm_weights(snr, 0.0, R, 2)[:2]
    return sm_weights(snr, 0.0, R, 2, detector)


def plan(detector, name, m, R):
    key = (plan_class(detector), name, m, R)
    if key not in _plans:
        _plans[key] = key[0](LinkConfig(sm_inputs(name)[0], m), DEV, R)
    return _plans[key]


def operands(detector, name, R, which="lmmse"):
    """The frames whole groups of 2 R fill, on the host and on the device: (n, (ideal, est, keys, sigma, *weights)) twice, in the order
    the plan takes them."""
    if (detector, name, R, which) not in _ops:
        sim, keys, sigma, snr, ideal, est = sm_inputs(name)
        n = len(keys) // (2 * R) * 2 * R
        host = (ideal[:n], est[which][:n], keys[:n], sigma[:n], *weights(snr[:n], R, detector))
        _ops[detector, name, R, which] = (n, host, tuple(_dev(a) for a in host))
    return _ops[detector, name, R, which]


def run(detector, name, m, R, which="lmmse", want_llr=True, lib=None):
    return plan(detector, name, m, R)(*operands(detector, name, R, which)[2], _dev(FACTORS), want_llr=want_llr, lib=lib)


def entry_name(detector):
    return "aft_link_joint_f32" if detector == JOINT_DETECTOR else "aft_link_sm_f32"


def entry(detector, plan, ops, factors, counts, loss, llr, batch, hp=None, ep=None):
    h, e, *rest = ops
    return getattr(_lib.load(), entry_name(detector))(
        ctypes.byref(plan.link), hp or h.data_ptr(), ep or e.data_ptr(), *(t.data_ptr() for t in rest), factors.data_ptr(), factors.numel(),
        plan.branches, plan.streams, counts.data_ptr(), loss.data_ptr(), llr, batch, _lib.current_stream_ptr(counts.device))


def group_independence(m, cases):
    """``cases``: the (R, detector) pairs."""
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        sim, keys, sigma, snr, ideal, est = sm_inputs(name)
        for R, detector in cases:
            p, W = plan(detector, name, m, R), 2 * R
            idx = (np.arange(37 * W) * 5 + 1) % len(keys)                        # 37 groups of the same frames in another order ...
            idx[-W:] = np.arange(W, 2 * W)                                       # ... the last one group 1 of ``operands``
            ops = lambda i: (_dev(ideal[i]), _dev(est["lmmse"][i]), _dev(keys[i]), _dev(sigma[i]),  # noqa: E731
                             *(_dev(a) for a in weights(snr[i], R, detector)))
            batch = p(*ops(idx), f, want_llr=True)
            alone = p(*ops(np.arange(W, 2 * W)), f, want_llr=True)
            _same_bits([t[72:74] for t in batch], alone)
            _same_bits([t[2:4] for t in run(detector, name, m, R)], alone)       # second of the groups of ``operands``
            _same_bits(p(*ops(idx), f, want_llr=True), batch)                    # a second run of the same batch


def poisoned_outputs(detector, m):
    """Every element of the three outputs is written and nothing beside them; without the LLR output, and with ideal, est and llr 8, 4
    and 12 bytes off a 16-byte boundary (the 8-byte loads, the 8- and 4-byte stores), the same bits."""
    f = _dev(FACTORS)
    for name in ("default_120x14", "odd_30x7"):
        for R in (2, 3):
            n, _, ops = operands(detector, name, R)
            p, F = plan(detector, name, m, R), n // R
            want = run(detector, name, m, R)
            h, e = ops[0], ops[1]
            fh, fe = (torch.empty(h.numel() + 1, dtype=torch.complex64, device=DEV) for _ in range(2))
            fh[1:], fe[1:] = h.reshape(-1), e.reshape(-1)
            assert (fh.data_ptr() + 8) % 16 == 8 and (fe.data_ptr() + 8) % 16 == 8
            for hp, ep, off in ((None, None, 0), (fh.data_ptr() + 8, fe.data_ptr() + 8, 8), (None, fe.data_ptr() + 8, 0), (None, None, 8),
                                (None, None, 4), (fh.data_ptr() + 8, None, 12), (None, None, None)):
                counts = torch.full((F + 1, 2), POISON, dtype=torch.int32, device=DEV)
                loss = torch.full((F + 1, 3), float("nan"), device=DEV)
                llr = torch.full((want[2].numel() + 4,), float("nan"), device=DEV)
                _lib.check(entry(detector, p, ops, f, counts, loss, None if off is None else llr.data_ptr() + off, n, hp, ep))
                _same_bits([counts[:F], loss[:F]], want[:2])
                assert (counts[F:] == POISON).all() and loss[F:].isnan().all()
                if off is None:
                    assert llr.isnan().all()
                else:
                    at = off // 4
                    _same_bits([llr[at:at + want[2].numel()]], [want[2].reshape(-1)])
                    assert llr[:at].isnan().all() and llr[at + want[2].numel():].isnan().all()
            _same_bits(run(detector, name, m, R, want_llr=False)[:2], want[:2])
    # the odd grid whose last element (14, at (2, 4)) is data and alone in its pair: written for both streams, finite and not a pilot's zero
    n, _, ops = operands(detector, MRC_ODD, 2)
    counts = torch.full((2, 2), POISON, dtype=torch.int32, device=DEV)
    loss, llr = torch.full((2, 3), float("nan"), device=DEV), torch.full((2, 3, 5, m), float("nan"), device=DEV)
    _lib.check(entry(detector, plan(detector, MRC_ODD, m, 2), ops, f, counts, loss, llr.data_ptr(), n))
    _same_bits([counts, loss, llr], run(detector, MRC_ODD, m, 2))
    assert llr.isfinite().all() and (llr[:, 2, 4] != 0).all() and (llr[:, 1, 2] == 0).all()


def checked_build(cases):
    """``cases``: the (R, detector) pairs, all of one entry point."""
    symbol = entry_name(cases[0][1])
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), symbol):                 # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, symbol)
    for name in ("default_120x14", "odd_30x7"):
        for m in BITS_PER_SYMBOL:
            for R, detector in cases:
                _same_bits(run(detector, name, m, R, lib=lib), run(detector, name, m, R))
    for m in BITS_PER_SYMBOL:
        _same_bits(run(cases[0][1], MRC_ODD, m, 2, lib=lib), run(cases[0][1], MRC_ODD, m, 2))


def plan_refusals(detector):
    """The batch, then every operand after ``sigma`` too short, then the last of them with another dtype and in pageable host memory,
    then the factors: in the order the plan checks them."""
    n, _, (h, e, k, s, *w) = operands(detector, "odd_30x7", 4)
    p, f, names = plan(detector, "odd_30x7", 4, 4), _dev(FACTORS), ("rho", "scale", "reg")[:len(w)]
    swapped = lambda i, t: (h, e, k, s, *w[:i], t, *w[i + 1:], f)  # noqa: E731
    last = len(w) - 1
    for args, word in (((h[:6], e[:6], k[:6], s[:6], w[0][:6], *w[1:], f), "6 frames is not a multiple of branches \\* streams = 4 \\* 2"),
                       *((swapped(i, w[i][:8 if i == 0 else 3]), f"{names[i]} must hold") for i in range(len(w))),
                       (swapped(last, w[last].double()), f"{names[last]} must be torch.float32"),
                       (swapped(last, torch.from_numpy(np.zeros(4, np.float32))), "pinned host memory"),
                       ((h, e, k, s, *w, torch.ones(9, device=DEV)), "between 1 and 8")):
        with pytest.raises(ValueError, match=word):
            p(*args)
    cls = plan_class(detector)
    for bad in (0, 1, 9, 2.0, True):
        with pytest.raises(ValueError, match="branches"):
            cls(p.cfg, DEV, bad)
    for bad in (1, 3, 2.0, True):
        with pytest.raises(ValueError, match="streams"):
            cls(p.cfg, DEV, 2, bad)
    with pytest.raises(ValueError, match=f"{cls.__name__} runs on a HIP device"):
        cls(p.cfg, "cpu", 2)


def entry_refusals(detector):
    name, m, R = "default_120x14", 4, 2
    n, _, (h, e, k, s, *w) = operands(detector, name, R)
    lib, F, f = _lib.load(), n // R, _dev(FACTORS)
    fn, words = getattr(lib, entry_name(detector)), ("rho", "scale", "reg")[:len(w)]
    cfg = LinkConfig(sm_inputs(name)[0], m)
    counts = torch.full((F, 2), POISON, dtype=torch.int32, device=DEV)
    loss = torch.full((F, 3), float("nan"), device=DEV)
    llr = torch.full((F, *cfg.sim.ofdm, m), float("nan"), device=DEV)
    good = dict(ideal=h.data_ptr(), est=e.data_ptr(), keys=k.data_ptr(), sigma=s.data_ptr(), **{x: t.data_ptr() for x, t in zip(words, w)},
                factors=f.data_ptr(), n_factors=3, branches=R, streams=2, counts=counts.data_ptr(), loss=loss.data_ptr(),
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
    for x in ("ideal", "est", "keys", "sigma", *words, "factors", "counts", "loss"):
        refused(E, "NULL pointer", **{x: None})
    for x in ("ideal", "est", "keys"):
        refused(E, "8-byte", **{x: good[x] + 4})
    for x in ("sigma", *words, "factors", "counts", "loss", "llr"):
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
    _same_bits([counts, loss, llr], run(detector, name, m, R))                       # ... and the good call writes it all
    # a grid whose every element is a pilot is legal: counts 0, loss 0, LLR 0
    one = LinkConfig(ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1)), m).to_struct()
    assert call(one, batch=4) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert counts[:2].tolist() == [[0, 0]] * 2 and loss[:2].tolist() == [[0.0] * 3] * 2 and llr.reshape(-1)[:2 * m].tolist() == [0.0] * (2 * m)


def coded_accumulators(kind, detector):
    R, N, seed = 2, 2, 2
    sim = ChannelSimConfig()
    link = LinkConfig(sim, 4)
    code = CodeConfig(link, 256, "3/4") if kind == "viterbi" else LdpcConfig(link, "1/2")
    make = BlockErrorAccumulator if kind == "viterbi" else LdpcBlockErrorAccumulator
    decode = link_decode_host if kind == "viterbi" else link_ldpc_host
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=seed)
    with_est, perfect, on_device = (make(code, DEV, seed=seed, branches=R, streams=N, detector=detector) for _ in range(3))
    assert type(with_est._plan) is plan_class(detector)
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
    p, one = plan_class(detector)(link, DEV, R), torch.ones(1, device=DEV)
    want = np.zeros((2, len(with_est.errors)), np.int64)
    for ideal, est, meta in seen:
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        sent_keys = np.ascontiguousarray(keys.reshape(-1, R, N)[:, 0, :]).reshape(-1)
        w = tuple(_dev(a) for a in weights(snr, R, detector))
        for i, e in enumerate((est, ideal)):
            _, _, llr = p(ideal, e, _dev(keys), _dev(noise_sigma(snr)), *w, one, want_llr=True)
            want[i] += decode(code, sent_keys, llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()     # keys hashed on the device are the host's
    assert with_est.result() == want[0][1] / (rows * code.blocks) and perfect.result() <= with_est.result()
    print(f"{kind}, 2 x 2 {detector}: BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}")
