"""``aft_link_decode_f32``, ``hip_ops.LinkDecodePlan``, ``linksim.BlockErrorAccumulator`` and ``evaluation.get_link_bler`` on the HIP
device.  Everything after the quantiser is integer and the quantiser is one float32 product rounded to nearest even, so the kernel's
counts and decoded bits are compared with ``linksim.link_decode_host`` on the same float32 LLR tensor for EQUALITY: no tolerance.

A batch of five frames per case: two frames of LLRs from ``aft_link_soft_f32`` (LS-interpolated estimates), one of random small
multiples of 1/8 (many ties), one of zeros (the tie rule decides everything), one of saturating values, infinities and NaN.  The step
counts K + 6 are 7, 63, 64, 65, 127, 128, 129 (around the 64 steps a wave prepares at once) and 4096 (the bound: a block's survivor
words are 32 KiB of LDS); all three rates and all four modulation orders; grids with an odd T, with pilots on
the first and the last grid element, and with pilot rows that hold no data element."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, simulate_frames_host
from adafortitran_amd.hip_ops import LinkDecodePlan, LinkSoftPlan
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, RATES, BlockErrorAccumulator, CodeConfig, LinkConfig, link_decode_host, llr_scale,
                                      noise_sigma)
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync
from test_linkcode import SEED, SIMS, sanity_inputs
from test_linksim_gpu import _dev, _pinned

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMES = 5
SPECIAL = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 15.875, -15.875, 15.9376, -15.9376, 0.0625, -0.0625, 0.1875, -0.3125, 100.0, 0.0,
                    -0.0, 3.4e38, 1e-40], dtype=np.float32)
_frames, _llrs = {}, {}


def _soft_llrs(sim: ChannelSimConfig, m: int, frames=2) -> torch.Tensor:
    """float32 ``[frames, S, T, m]`` on the device: what aft_link_soft_f32 writes for frames of SEED with LS-interpolated estimates."""
    key = (sim.ofdm, sim.pilot_scs, sim.pilot_symbols)
    if key not in _frames:
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(frames))
        _frames[key] = (ideal.astype(np.complex64), ls_interpolate(sim, pilots.astype(np.complex64)), meta)
    ideal, est, meta = _frames[key]
    keys = frame_keys(SEED, np.arange(frames))
    _, llr = LinkSoftPlan(LinkConfig(sim, m), DEV)(_dev(ideal), _dev(est), _dev(keys), _dev(noise_sigma(meta[:, 0])),
                                                   _dev(llr_scale(meta[:, 0])), torch.ones(1, device=DEV), want_llr=True)
    return llr


def case_llrs(sim: ChannelSimConfig, m: int) -> torch.Tensor:
    """The five frames of a case (module docstring), made once per grid and modulation order."""
    key = (sim.ofdm, sim.pilot_scs, sim.pilot_symbols, m)
    if key not in _llrs:
        rng = np.random.default_rng(17 + m)
        shape = (*sim.ofdm, m)
        eighths = (rng.integers(-4, 5, shape) / 8.0).astype(np.float32)
        special = SPECIAL[rng.integers(0, len(SPECIAL), shape)]
        host = torch.from_numpy(np.stack([eighths, np.zeros(shape, np.float32), special]))
        _llrs[key] = torch.cat([_soft_llrs(sim, m), host.to(DEV)]).contiguous()
    return _llrs[key]


KEYS = frame_keys(SEED, np.arange(FRAMES))


def _decode_poisoned(code: CodeConfig, llr: torch.Tensor, keys: torch.Tensor, want_bits=True, lib=None):
    """The entry point itself on outputs filled with values no decoder writes."""
    lib = lib or _lib.load()
    b = llr.shape[0]
    counts = torch.full((b, 2), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((b, code.blocks, code.info_bits), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.aft_link_decode_f32(ctypes.byref(code.link.to_struct()), llr.data_ptr(), keys.data_ptr(), code.info_bits, code.rate_code,
                                       code.stride, code.stride_inverse, code.qgain, counts.data_ptr(), bits.data_ptr() if want_bits else None,
                                       b, _lib.current_stream_ptr(llr.device)), lib)
    return counts, bits


def _equal_to_the_host(code: CodeConfig, llr: torch.Tensor, keys: np.ndarray = KEYS, lib=None):
    want_counts, want_bits = link_decode_host(code, keys, llr.cpu().numpy())
    counts, bits = _decode_poisoned(code, llr, _dev(keys), lib=lib)
    assert bits.max().item() <= 1                                                # every element was written
    assert counts.cpu().tolist() == want_counts.tolist(), (code.info_bits, code.rate, code.link.bits_per_symbol)
    assert torch.equal(bits.cpu(), torch.from_numpy(want_bits))
    bare, untouched = _decode_poisoned(code, llr, _dev(keys), want_bits=False, lib=lib)     # bits = NULL: the same counts
    assert torch.equal(bare, counts) and (untouched == 0xAB).all()
    return want_counts


def _code_that_fits(K, rate, m, turn):
    names = ("odd_30x7", "edges_24x6", "full_rows_40x2")
    for i in range(3):
        sim = SIMS[names[(turn + i) % 3]]
        try:
            return CodeConfig(LinkConfig(sim, m), K, rate)
        except ValueError:                                                       # B = 0 on this grid: the next one
            continue
    raise AssertionError((K, rate, m))


@pytest.mark.parametrize("K", (1, 57, 58, 59, 121, 122, 123))
def test_counts_and_bits_equal_the_host_decoder(K):
    turn, grids, errors = 0, set(), 0
    for rate in RATES:
        for m in BITS_PER_SYMBOL:
            code = _code_that_fits(K, rate, m, turn)
            turn += 1
            grids.add(code.link.sim.ofdm)
            errors += int(_equal_to_the_host(code, case_llrs(code.link.sim, m))[:, 0].sum())
    assert len(grids) >= 2 and errors > 0                                        # zeros and garbage do not decode to the sent bits


@pytest.mark.parametrize("rate,m,scs,blocks", (("1/2", 8, 120, 1), ("2/3", 8, 120, 2), ("3/4", 8, 120, 2), ("3/4", 6, 120, 1), ("3/4", 8, 200, 4)))
def test_the_4096_step_bound(rate, m, scs, blocks):
    """K = 4090 on the default grid: at rate 1/2 and m = 8 one block of 8192 coded bits and 5056 bits of filler.  On 200 x 14 four
    blocks: four waves, whose survivor words are 128 KiB, the most a workgroup asks for."""
    code = CodeConfig(LinkConfig(ChannelSimConfig(ofdm=(scs, 14)), m), 4090, rate)
    assert code.steps == 4096 and code.blocks == blocks
    assert code.used_bits < code.link.bits_per_frame
    _equal_to_the_host(code, case_llrs(code.link.sim, m))


def test_more_blocks_than_waves_and_a_given_stride():
    """111 blocks of 14 coded bits over 16 waves (the last round is ragged); B = 1 with filler; strides that are not the default; a
    quantiser gain that is not 8."""
    code = CodeConfig(LinkConfig(SIMS["odd_30x7"], 8), 1, "1/2")
    assert code.blocks == 111
    _equal_to_the_host(code, case_llrs(code.link.sim, 8))
    one = CodeConfig(LinkConfig(SIMS["edges_24x6"], 2), 100, "1/2")
    assert one.blocks == 1 and one.used_bits == 212 < one.link.bits_per_frame == 276
    _equal_to_the_host(one, case_llrs(one.link.sim, 2))
    for stride in (1, 211, 5):
        given = CodeConfig(LinkConfig(SIMS["edges_24x6"], 2), 100, "1/2", stride=stride)
        _equal_to_the_host(given, case_llrs(given.link.sim, 2))
    coarse = CodeConfig(LinkConfig(SIMS["odd_30x7"], 4), 40, "3/4", qgain=0.75)
    _equal_to_the_host(coarse, case_llrs(coarse.link.sim, 4))


def test_a_frame_does_not_depend_on_its_batch_its_position_or_the_run():
    code = CodeConfig(LinkConfig(SIMS["odd_30x7"], 4), 59, "2/3")
    plan = LinkDecodePlan(code, DEV)
    five = case_llrs(code.link.sim, 4)
    order = [3, 0, 4, 4, 1, 2, 0, 0, 3, 1, 2]
    llr, keys = five[order].contiguous(), _dev(KEYS[order])
    counts, bits = plan(llr, keys, want_bits=True)
    assert counts.shape == (11, 2) and counts.dtype == torch.int32 and bits.shape == (11, code.blocks, 59) and bits.dtype == torch.uint8
    alone = [plan(five[i:i + 1], _dev(KEYS[i:i + 1]), want_bits=True) for i in range(FRAMES)]
    for at, i in enumerate(order):
        assert torch.equal(counts[at:at + 1], alone[i][0]) and torch.equal(bits[at:at + 1], alone[i][1])
    again = plan(llr, keys, want_bits=True)
    assert torch.equal(again[0], counts) and torch.equal(again[1], bits)
    bare, none = plan(llr, keys)
    assert none is None and torch.equal(bare, counts)


def test_keys_in_pinned_memory_and_what_the_plan_refuses():
    code = CodeConfig(LinkConfig(SIMS["edges_24x6"], 6), 57, "3/4")
    plan = LinkDecodePlan(code, DEV)
    llr = case_llrs(code.link.sim, 6)
    want = plan(llr, _dev(KEYS), want_bits=True)
    got = plan(llr, _pinned(KEYS).reshape(-1, 1), want_bits=True)                # read in place
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    kd = _dev(KEYS)
    for args, word in (((llr, torch.from_numpy(KEYS.view(np.int64).copy())), "pinned host memory"), ((llr, kd[:3]), "one value per frame"),
                       ((llr, kd.to(torch.int32)), "keys must be torch.int64"), ((llr.double(), kd), "llr must be float32"),
                       ((llr[:, :, :3], kd), "Expected llr shape"), ((llr[..., :4], kd), "Expected llr shape"), ((llr[:0], kd[:0]), "Expected llr shape"),
                       ((llr.cpu(), kd), "must live on")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    with pytest.raises(ValueError, match="LinkDecodePlan runs on a HIP device"):
        LinkDecodePlan(code, "cpu")
    with pytest.raises(ValueError, match="LinkDecodePlan needs a linksim.CodeConfig"):
        LinkDecodePlan(code.link, DEV)


def test_every_refusal_of_the_entry_point_launches_nothing():
    code = CodeConfig(LinkConfig(SIMS["odd_30x7"], 4), 59, "1/2")               # n = 130, B = 6, U = 780
    assert (code.coded_bits, code.blocks, code.used_bits) == (130, 6, 780)
    lib = _lib.load()
    llr, keys = case_llrs(code.link.sim, 4), _dev(KEYS)
    counts = torch.full((FRAMES, 2), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((FRAMES, 6, 59), 0xAB, dtype=torch.uint8, device=DEV)
    good = dict(llr=llr.data_ptr(), keys=keys.data_ptr(), info_bits=59, rate=code.rate_code, stride=code.stride,
                stride_inverse=code.stride_inverse, qgain=8.0, counts=counts.data_ptr(), bits=bits.data_ptr(), batch=FRAMES)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = code.link.to_struct() if p is None else p
        return lib.aft_link_decode_f32(ctypes.byref(p), *(a[n] for n in good), None)

    def refused(rc_want, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == rc_want and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error(), kw)

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_decode_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for name in ("llr", "keys", "counts"):
        refused(E, "NULL pointer", **{name: None})
    refused(E, "8-byte", keys=good["keys"] + 4)
    for name in ("llr", "counts"):
        refused(E, "4-byte", **{name: good[name] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for qgain in (0.0, -8.0, float("inf"), float("nan")):
        refused(E, "finite and positive", qgain=qgain)
    for k in (0, -1, 4091, 1 << 20):
        refused(SH, f"info_bits = {k} is outside 1..4090", info_bits=k)
    for rate in (-1, 3, 133):
        refused(SH, f"rate = {rate}", rate=rate)
    refused(SH, "fewer than the 794 coded bits", info_bits=391)                  # 780 bits per frame
    for stride in (0, 780, 781, 1 << 40):
        refused(SH, "is outside [1, 780)", stride=stride)
    for stride in (2, 13, 390):
        refused(SH, "not coprime", stride=stride)
    for inverse in (0, 780, code.stride_inverse + 1, 1):
        refused(SH, "is not the inverse", stride_inverse=inverse)

    def struct(**fields):
        p = code.link.to_struct()
        for name, value in fields.items():
            setattr(p, name, value)
        return p

    for fields, word in ((dict(num_scs=0), "num_scs = 0"), (dict(num_symbols=-1), "num_symbols = -1"),
                         (dict(num_scs=1 << 16, num_symbols=(1 << 15) + 1), "more than 2^31 elements"),
                         (dict(pilot_scs=65), "pilot_scs = 65 is outside 1..64"), (dict(pilot_symbols=0), "pilot_symbols = 0"),
                         (dict(num_symbols=2), "larger than the ofdm grid"), (dict(bits_per_symbol=3), "bits_per_symbol = 3"),
                         (dict(bits_per_symbol=10), "bits_per_symbol = 10")):
        refused(SH, word, p=struct(**fields))
    torch.cuda.synchronize()
    assert (counts == -7).all() and (bits == 0xAB).all()                         # nothing was launched
    assert call() == _abi.AFT_OK and call(bits=None) == _abi.AFT_OK              # a NULL bits is legal
    torch.cuda.synchronize()
    want_counts, want_bits = link_decode_host(code, KEYS, llr.cpu().numpy())
    assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_decode_f32"):   # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_decode_f32")
    for name, m, rate, K in (("odd_30x7", 4, "3/4", 59), ("edges_24x6", 8, "1/2", 122), ("full_rows_40x2", 2, "2/3", 58), ("odd_30x7", 6, "2/3", 1)):
        code = CodeConfig(LinkConfig(SIMS[name], m), K, rate)
        _equal_to_the_host(code, case_llrs(code.link.sim, m), lib=lib)
    big = CodeConfig(LinkConfig(ChannelSimConfig(), 8), 4090, "3/4")
    _equal_to_the_host(big, case_llrs(big.link.sim, 8), lib=lib)


def test_physical_sanity_on_the_device():
    """20 dB, 16-QAM, rate 1/2, K = 512, 24 blocks: perfect channel knowledge has no block error, the LS estimate has some, and both
    equal the host decoder on the device's own LLRs (which differ from the float64 ones in the quantiser's last step)."""
    code, keys, sigma, scale, ideal, est = sanity_inputs()
    soft, plan = LinkSoftPlan(code.link, DEV), LinkDecodePlan(code, DEV)
    blocks = {}
    for which, e in est.items():
        _, llr = soft(_dev(ideal), _dev(e), _dev(keys), _dev(sigma), _dev(scale), torch.ones(1, device=DEV), want_llr=True)
        counts, bits = plan(llr, _dev(keys), want_bits=True)
        want_counts, want_bits = link_decode_host(code, keys, llr.cpu().numpy())
        assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))
        blocks[which] = int(counts[:, 1].sum())
    print("block errors of 24:", blocks)
    assert blocks["ideal"] == 0 and blocks["ls"] >= 1


def test_block_error_accumulator_runs_from_the_loader_without_a_synchronisation():
    sim = ChannelSimConfig()
    code = CodeConfig(LinkConfig(sim, 4), 256, "3/4")
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=2)
    with_est, perfect, on_device = (BlockErrorAccumulator(code, DEV, seed=2) for _ in range(3))
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
    assert len(seen) == 3 and with_est.frames == perfect.frames == 48 and with_est.errors.is_cuda and with_est.errors.dtype == torch.int64
    # what the accumulator launched, step by step: the soft plan's LLRs through the host decoder
    soft = LinkSoftPlan(code.link, DEV)
    want = np.zeros((2, 2), np.int64)
    for ideal, est, meta in seen:
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(2, g)
        for i, e in enumerate((est, ideal)):
            _, llr = soft(ideal, e, _dev(keys), _dev(noise_sigma(snr)), _dev(llr_scale(snr)), torch.ones(1, device=DEV), want_llr=True)
            want[i] += link_decode_host(code, keys, llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    blocks = 48 * code.blocks
    assert with_est.result() == want[0][1] / blocks and with_est.result_ber() == want[0][0] / (blocks * 256)
    assert perfect.result_throughput() == pytest.approx((blocks - want[1][1]) * 256 / (48 * code.link.data_elements))
    assert perfect.result() <= with_est.result()
    # keys hashed with torch ops on the device are the host's, and the SNRs came from the host both times: the same integers
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()
    print(f"BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}")


def test_bler_sweep_over_simulated_packs():
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import make_pack
    from adafortitran_amd.evaluation import get_link_bler
    sim = ChannelSimConfig()
    code = CodeConfig(LinkConfig(sim, 4), 512, "1/2")
    packs = {snr: make_pack(sim, 32, seed=20 + snr, snr_db=snr) for snr in (5, 25)}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, sim.pilot, 16, device=DEV, shuffle=False)) for snr, pack in packs.items()]
    perfect = get_link_bler(None, loaders, code, seed=1)
    lmmse = get_link_bler(LmmseEstimator(sim).to(DEV), loaders, code, seed=1)
    print("BLER with the channel", perfect, " with the LMMSE estimate", lmmse)
    assert list(perfect) == list(lmmse) == [5, 25]
    assert 0 <= perfect[25] <= perfect[5] <= 1 and perfect[25] <= lmmse[25] and perfect[25] < 0.5 < perfect[5]
