"""``aft_link_ldpc_f32``, ``hip_ops.LinkLdpcPlan``, ``linksim.LdpcBlockErrorAccumulator`` and ``evaluation.get_link_bler`` with an
``LdpcConfig`` on the HIP device.  Everything after the quantiser is integer and the quantiser is one float32 product rounded to
nearest even, so the kernel's three counts and its decoded bits are compared with ``linksim.link_ldpc_host`` on the same float32 LLR
tensor for EQUALITY: no tolerance.

A batch of five frames per case, those of tests/test_linkcode_gpu.py: two frames of LLRs from ``aft_link_soft_f32`` (LS-interpolated
estimates), one of random small multiples of 1/8 (many ties), one of zeros (every block stops after one iteration with all-zero
bits), one of saturating values, infinities and NaN (which does not converge and runs into ``max_iters``)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkLdpcPlan, LinkSoftPlan, fill_lds
from adafortitran_amd.linksim import BITS_PER_SYMBOL, LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig, link_ldpc_host, llr_scale, noise_sigma
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync
from test_linkcode import SEED, SIMS, sanity_inputs
from test_linkcode_gpu import FRAMES, KEYS, case_llrs
from test_linksim_gpu import _dev, _pinned

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEFAULT = ChannelSimConfig()
ZEROS, SPECIALS = 3, 4                                       # the frame of zeros and the frame of specials in a case's batch


def _decode_poisoned(cfg: LdpcConfig, llr: torch.Tensor, keys: torch.Tensor, want_bits=True, lib=None):
    """The entry point itself on outputs filled with values no decoder writes."""
    lib = lib or _lib.load()
    b = llr.shape[0]
    counts = torch.full((b, 3), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((b, cfg.blocks, cfg.info_bits), 0xAB, dtype=torch.uint8, device=DEV)
    shifts = np.ascontiguousarray(cfg.shifts, dtype=np.int32)
    _lib.check(lib.aft_link_ldpc_f32(ctypes.byref(cfg.link.to_struct()), llr.data_ptr(), keys.data_ptr(), cfg.base_rows, cfg.base_cols,
                                     shifts.ctypes.data, cfg.stride, cfg.stride_inverse, cfg.qgain, cfg.offset, cfg.max_iters,
                                     counts.data_ptr(), bits.data_ptr() if want_bits else None, b, _lib.current_stream_ptr(llr.device)), lib)
    return counts, bits


def _equal_to_the_host(cfg: LdpcConfig, llr: torch.Tensor, keys: np.ndarray = KEYS, lib=None):
    want_counts, want_bits = link_ldpc_host(cfg, keys, llr.cpu().numpy())
    counts, bits = _decode_poisoned(cfg, llr, _dev(keys), lib=lib)
    assert bits.max().item() <= 1                                                # every element was written
    assert counts.cpu().tolist() == want_counts.tolist(), (cfg.rate, cfg.link.bits_per_symbol)
    assert torch.equal(bits.cpu(), torch.from_numpy(want_bits))
    bare, untouched = _decode_poisoned(cfg, llr, _dev(keys), want_bits=False, lib=lib)      # bits = NULL: the same counts
    assert torch.equal(bare, counts) and (untouched == 0xAB).all()
    return want_counts


def _on(sim: ChannelSimConfig, m: int, rate, **kw):
    cfg = LdpcConfig(LinkConfig(sim, m), rate, **kw)
    return cfg, case_llrs(sim, m)


def test_the_smallest_code_one_block_with_filler_and_six_blocks():
    one, llr = _on(SIMS["odd_30x7"], 2, (3, 4))
    assert one.blocks == 1 and one.used_bits == 256 < one.link.bits_per_frame == 390
    assert _equal_to_the_host(one, llr)[ZEROS, 2] == 1
    six, llr = _on(SIMS["odd_30x7"], 8, (3, 4))
    assert six.blocks == 6 and six.used_bits == 1536 < 1560
    counts = _equal_to_the_host(six, llr)
    assert counts[ZEROS, 2] == 6 and counts[SPECIALS, 2] > 6 and counts[:, 0].sum() > 0


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_all_modulation_orders_on_the_small_grids(m):
    grids = 0
    for name, rate in (("odd_30x7", (3, 4)), ("edges_24x6", (3, 4)), ("full_rows_40x2", (3, 4)), ("odd_30x7", (4, 6)), ("edges_24x6", (5, 8))):
        try:
            cfg, llr = _on(SIMS[name], m, rate)
        except ValueError:                                                       # B = 0 on this grid at this order
            continue
        grids += 1
        _equal_to_the_host(cfg, llr)
    assert grids >= 3


@pytest.mark.parametrize("rate", ("1/2", "2/3", "3/4"))
def test_the_rate_presets_at_every_order(rate):
    cfg, llr = _on(SIMS["odd_30x7"], 8, rate)                                    # n = 1536 of the grid's 1560 bits
    assert cfg.blocks == 1
    _equal_to_the_host(cfg, llr)
    for m in BITS_PER_SYMBOL:
        cfg, llr = _on(DEFAULT, m, rate)
        assert cfg.blocks == m and cfg.coded_bits == 1536
        _equal_to_the_host(cfg, llr)


@pytest.mark.parametrize("rate,edges", (((3, 32), 94), ((16, 32), 81)))
def test_the_widest_row_and_the_tallest_base_matrix(rate, edges):
    """3 x 32: row degree 32, the most edges a row has.  16 x 32: the most layers and parity words."""
    cfg, llr = _on(DEFAULT, 4, rate)
    assert cfg.edges == edges and cfg.blocks == 3 and cfg.coded_bits == 2048
    assert max(len(cols) for cols, _ in cfg.layers()) == (32 if rate == (3, 32) else 6)
    _equal_to_the_host(cfg, llr)


def test_more_blocks_than_waves():
    cfg, llr = _on(DEFAULT, 8, (3, 4))
    assert cfg.blocks == 51                                                      # 16 waves: three full rounds and one of three
    assert _equal_to_the_host(cfg, llr)[ZEROS, 2] == 51


def test_the_most_edges_share_the_lds_between_fewer_waves():
    """160 entries and n = 2048: 14 KiB per block, so ten blocks in flight of the thirteen of a frame."""
    table = np.full((16, 16), -1, np.int32)
    rng = np.random.default_rng(2)
    table[:8, :] = rng.integers(0, 64, (8, 16))
    table[7, 0] = -1
    cfg = LdpcConfig(LinkConfig(ChannelSimConfig(ofdm=(240, 14)), 8), (16, 32), shifts=table, max_iters=4)
    assert cfg.edges == 160 and cfg.blocks == 13
    _equal_to_the_host(cfg, case_llrs(cfg.link.sim, 8))


def test_a_user_table_with_shifts_0_and_63_and_a_column_of_weight_1():
    table = [[0, -1, 63], [63, -1, 0], [-1, 7, 0], [5, -1, -1]]
    cfg, llr = _on(SIMS["odd_30x7"], 8, (4, 7), shifts=table)
    assert cfg.blocks == 3 and cfg.edges == 7 + 9 and cfg.base()[:, 1].tolist() == [-1, -1, 7, -1]
    _equal_to_the_host(cfg, llr)


def test_one_iteration_the_cap_and_the_offsets():
    sim = SIMS["odd_30x7"]
    once, llr = _on(sim, 8, (3, 4), max_iters=1)
    assert _equal_to_the_host(once, llr)[:, 2].tolist() == [6] * FRAMES          # every block ran exactly one iteration
    capped, _ = _on(sim, 8, (3, 4), max_iters=7)
    counts = _equal_to_the_host(capped, llr)
    assert counts[SPECIALS, 2] == 6 * 7 and counts[ZEROS, 2] == 6                 # garbage runs into the cap, zeros stop at once
    longest, _ = _on(sim, 8, (3, 4), max_iters=255)
    assert _equal_to_the_host(longest, llr)[SPECIALS, 2] > 6 * 20
    for offset in (0, 127):
        cfg, _ = _on(sim, 8, (4, 6), offset=offset)
        _equal_to_the_host(cfg, llr)


def test_gains_that_saturate_the_quantiser_and_that_leave_it_coarse():
    """qgain = 1e4 puts every input that is neither 0 nor NaN at +-127; qgain = 0.75 leaves a handful of levels."""
    for qgain in (1e4, 0.75):
        cfg, llr = _on(SIMS["odd_30x7"], 8, (3, 4), qgain=qgain, max_iters=60)
        _equal_to_the_host(cfg, llr)


def test_given_strides():
    for stride in (1, 255, 5, 77):
        cfg, llr = _on(SIMS["odd_30x7"], 2, (3, 4), stride=stride)
        _equal_to_the_host(cfg, llr)
    cfg, llr = _on(DEFAULT, 6, "2/3", stride=9215)                               # U = 9216
    _equal_to_the_host(cfg, llr)


def test_a_frame_does_not_depend_on_its_batch_its_position_or_the_run():
    cfg, five = _on(SIMS["odd_30x7"], 8, (4, 6))
    plan = LinkLdpcPlan(cfg, DEV)
    order = [3, 0, 4, 4, 1, 2, 0, 0, 3, 1, 2]
    llr, keys = five[order].contiguous(), _dev(KEYS[order])
    counts, bits = plan(llr, keys, want_bits=True)
    assert counts.shape == (11, 3) and counts.dtype == torch.int32 and bits.shape == (11, cfg.blocks, 128) and bits.dtype == torch.uint8
    alone = [plan(five[i:i + 1], _dev(KEYS[i:i + 1]), want_bits=True) for i in range(FRAMES)]
    for at, i in enumerate(order):
        assert torch.equal(counts[at:at + 1], alone[i][0]) and torch.equal(bits[at:at + 1], alone[i][1])
    again = plan(llr, keys, want_bits=True)
    assert torch.equal(again[0], counts) and torch.equal(again[1], bits)
    bare, none = plan(llr, keys)
    assert none is None and torch.equal(bare, counts)


def test_keys_in_pinned_memory_and_what_the_plan_refuses():
    cfg, llr = _on(SIMS["edges_24x6"], 6, (3, 4))
    plan = LinkLdpcPlan(cfg, DEV)
    want = plan(llr, _dev(KEYS), want_bits=True)
    got = plan(llr, _pinned(KEYS).reshape(-1, 1), want_bits=True)                # read in place
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    host = link_ldpc_host(cfg, KEYS, llr.cpu().numpy())
    assert want[0].cpu().tolist() == host[0].tolist() and torch.equal(want[1].cpu(), torch.from_numpy(host[1]))
    kd = _dev(KEYS)
    for args, word in (((llr, torch.from_numpy(KEYS.view(np.int64).copy())), "pinned host memory"), ((llr, kd[:3]), "one value per frame"),
                       ((llr, kd.to(torch.int32)), "keys must be torch.int64"), ((llr.double(), kd), "llr must be float32"),
                       ((llr[:, :, :3], kd), "Expected llr shape"), ((llr[..., :4], kd), "Expected llr shape"), ((llr[:0], kd[:0]), "Expected llr shape"),
                       ((llr.cpu(), kd), "must live on")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    with pytest.raises(ValueError, match="LinkLdpcPlan runs on a HIP device"):
        LinkLdpcPlan(cfg, "cpu")
    with pytest.raises(ValueError, match="LinkLdpcPlan needs a linksim.LdpcConfig"):
        LinkLdpcPlan(cfg.link, DEV)


def test_every_refusal_of_the_entry_point_launches_nothing():
    cfg, llr = _on(SIMS["odd_30x7"], 4, (3, 5))                                  # n = 320, B = 2, U = 640 of 780 bits
    assert (cfg.coded_bits, cfg.blocks, cfg.used_bits, cfg.info_bits) == (320, 2, 640, 128)
    lib = _lib.load()
    keys = _dev(KEYS)
    counts = torch.full((FRAMES, 3), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((FRAMES, 2, 128), 0xAB, dtype=torch.uint8, device=DEV)
    table = np.ascontiguousarray(cfg.shifts, dtype=np.int32)
    good = dict(llr=llr.data_ptr(), keys=keys.data_ptr(), base_rows=3, base_cols=5, shifts=table.ctypes.data, stride=cfg.stride,
                stride_inverse=cfg.stride_inverse, qgain=8.0, offset=4, max_iters=20, counts=counts.data_ptr(), bits=bits.data_ptr(),
                batch=FRAMES)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = cfg.link.to_struct() if p is None else p
        return lib.aft_link_ldpc_f32(ctypes.byref(p), *(a[n] for n in good), None)

    def refused(rc_want, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == rc_want and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error(), kw)

    def with_table(rows, cols, values):
        t = np.ascontiguousarray(values, dtype=np.int32).reshape(rows, cols - rows)
        return dict(base_rows=rows, base_cols=cols, shifts=t.ctypes.data), t        # the array is held by the caller

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_ldpc_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for name in ("llr", "keys", "shifts", "counts"):
        refused(E, "NULL pointer", **{name: None})
    refused(E, "8-byte", keys=good["keys"] + 4)
    for name in ("llr", "shifts", "counts"):
        refused(E, "4-byte", **{name: good[name] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for qgain in (0.0, -8.0, float("inf"), float("nan")):
        refused(E, "finite and positive", qgain=qgain)
    for rows in (2, 0, -1, 17):
        refused(SH, f"base_rows = {rows} is outside 3..16", base_rows=rows)
    for cols in (3, 2, 33, 1 << 20):
        refused(SH, f"base_cols = {cols} is outside 4..32", base_cols=cols)
    for offset in (-1, 128):
        refused(SH, f"offset = {offset} is outside 0..127", offset=offset)
    for iters in (0, -1, 256):
        refused(SH, f"max_iters = {iters} is outside 1..255", max_iters=iters)
    for bad in (-2, 64, 1 << 20):
        kw, held = with_table(3, 5, [[1, 2], [3, bad], [5, 6]])
        refused(SH, f"shifts[1][1] = {bad} is neither -1 nor a shift", **kw)
    kw, held = with_table(3, 5, [[1, -1], [3, -1], [5, -1]])
    refused(SH, "base column 1 has no entry", **kw)
    dense = np.full((16, 16), -1, np.int32)
    dense[:8, :] = 5
    kw, held = with_table(16, 32, dense)
    refused(SH, "161 entries", **kw)
    kw, held = with_table(3, 13, np.zeros((3, 10), np.int32))
    refused(SH, "fewer than the 832 coded bits", **kw)                           # 780 bits per frame
    for stride in (0, 640, 641, 1 << 40):
        refused(SH, "is outside [1, 640)", stride=stride)
    for stride in (2, 5, 320):
        refused(SH, "not coprime", stride=stride)
    for inverse in (0, 640, cfg.stride_inverse + 1, 1):
        refused(SH, "is not the inverse", stride_inverse=inverse)

    def struct(**fields):
        p = cfg.link.to_struct()
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
    want_counts, want_bits = link_ldpc_host(cfg, KEYS, llr.cpu().numpy())
    assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_ldpc_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_ldpc_f32")
    for name, m, rate in (("odd_30x7", 8, (3, 4)), ("edges_24x6", 6, (3, 4)), ("full_rows_40x2", 4, (3, 4)), ("odd_30x7", 8, "3/4")):
        cfg, llr = _on(SIMS[name], m, rate)
        _equal_to_the_host(cfg, llr, lib=lib)
    for m, rate in ((8, (3, 4)), (4, (3, 32)), (2, (16, 32))):
        cfg, llr = _on(DEFAULT, m, rate)
        _equal_to_the_host(cfg, llr, lib=lib)


@pytest.mark.parametrize("value", (float("nan"), 1e30, float("-inf")))
def test_the_bits_do_not_depend_on_what_the_lds_held(value):
    for sim, m, rate in ((SIMS["odd_30x7"], 8, (3, 4)), (DEFAULT, 4, "1/2"), (DEFAULT, 8, (3, 4))):
        cfg, llr = _on(sim, m, rate)
        plan = LinkLdpcPlan(cfg, DEV)
        want = plan(llr, _dev(KEYS), want_bits=True)
        fill_lds(value, "cuda:0")
        got = plan(llr, _dev(KEYS), want_bits=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    host = link_ldpc_host(cfg, KEYS, llr.cpu().numpy())
    assert got[0].cpu().tolist() == host[0].tolist() and torch.equal(got[1].cpu(), torch.from_numpy(host[1]))


def test_physical_sanity_on_the_device():
    """20 dB, 16-QAM, rate 1/2, 16 blocks: perfect channel knowledge has no block error, the LS estimate has some, and both equal the
    host decoder on the device's own LLRs (which differ from the float64 ones in the quantiser's last step)."""
    code, keys, sigma, scale, ideal, est = sanity_inputs()
    cfg = LdpcConfig(code.link, "1/2")
    soft, plan = LinkSoftPlan(cfg.link, DEV), LinkLdpcPlan(cfg, DEV)
    blocks = {}
    for which, e in est.items():
        _, llr = soft(_dev(ideal), _dev(e), _dev(keys), _dev(sigma), _dev(scale), torch.ones(1, device=DEV), want_llr=True)
        counts, bits = plan(llr, _dev(keys), want_bits=True)
        want_counts, want_bits = link_ldpc_host(cfg, keys, llr.cpu().numpy())
        assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))
        blocks[which] = counts[:, 1:].sum(dim=0).tolist()
    print("(block errors, iterations) of 16 blocks:", blocks)
    assert blocks["ideal"][0] == 0 and blocks["ls"][0] >= 1 and blocks["ideal"][1] < blocks["ls"][1]


def test_ldpc_accumulator_runs_from_the_loader_without_a_synchronisation():
    sim = ChannelSimConfig()
    cfg = LdpcConfig(LinkConfig(sim, 4), "3/4")
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=2)
    with_est, perfect, on_device = (LdpcBlockErrorAccumulator(cfg, DEV, seed=2) for _ in range(3))
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
    assert with_est.errors.shape == (3,)
    # what the accumulator launched, step by step: the soft plan's LLRs through the host decoder
    soft = LinkSoftPlan(cfg.link, DEV)
    want = np.zeros((2, 3), np.int64)
    for ideal, est, meta in seen:
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(2, g)
        for i, e in enumerate((est, ideal)):
            _, llr = soft(ideal, e, _dev(keys), _dev(noise_sigma(snr)), _dev(llr_scale(snr)), torch.ones(1, device=DEV), want_llr=True)
            want[i] += link_ldpc_host(cfg, keys, llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    blocks = 48 * cfg.blocks
    assert with_est.result() == want[0][1] / blocks and with_est.result_ber() == want[0][0] / (blocks * cfg.info_bits)
    assert with_est.result_iterations() == want[0][2] / blocks and 1 <= perfect.result_iterations() <= 20
    assert perfect.result_throughput() == pytest.approx((blocks - want[1][1]) * cfg.info_bits / (48 * cfg.link.data_elements))
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()
    print(f"BLER with the LMMSE estimate {with_est.result():.3f}, with the channel {perfect.result():.3f}; iterations "
          f"{with_est.result_iterations():.2f} and {perfect.result_iterations():.2f}")


def test_bler_sweep_over_simulated_packs():
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import make_pack
    from adafortitran_amd.evaluation import get_link_bler
    sim = ChannelSimConfig()
    cfg = LdpcConfig(LinkConfig(sim, 4), "1/2")
    packs = {snr: make_pack(sim, 32, seed=20 + snr, snr_db=snr) for snr in (5, 25)}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, sim.pilot, 16, device=DEV, shuffle=False)) for snr, pack in packs.items()]
    perfect = get_link_bler(None, loaders, cfg, seed=1)
    lmmse = get_link_bler(LmmseEstimator(sim).to(DEV), loaders, cfg, seed=1)
    print("BLER with the channel", perfect, " with the LMMSE estimate", lmmse)
    assert list(perfect) == list(lmmse) == [5, 25]
    assert 0 <= perfect[25] <= perfect[5] <= 1 and perfect[25] <= lmmse[25] and perfect[25] < 0.5 < perfect[5]
