"""``aft_link_harq_f32``, ``hip_ops.LinkHarqPlan``, ``linksim.HarqAccumulator`` and ``evaluation.get_link_harq`` on the HIP device.
Everything after the quantiser is integer and the quantiser is one float32 product rounded to nearest even, so the kernel's seven
counts and its decoded bits are compared with ``linksim.link_harq_host`` on the same float32 LLR tensor for EQUALITY: no tolerance.

The LLR frames are the five of tests/test_linkcode_gpu.py (two frames from ``aft_link_soft_f32`` with LS-interpolated estimates, one
of ties, one of zeros, one of saturating values, infinities and NaN), regrouped by index with their own keys: a frame may be the
round of several groups, and several rounds of one."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys
from adafortitran_amd.hip_ops import LinkHarqPlan, LinkLdpcPlan, LinkSoftPlan, fill_lds
from adafortitran_amd.linksim import HarqAccumulator, HarqConfig, LdpcConfig, LinkConfig, link_harq_host, llr_scale, noise_sigma
from adafortitran_amd.lmmse import LmmseEstimator
from test_chansim_gpu import _no_sync
from test_linkcode import SIMS
from test_linkcode_gpu import KEYS, case_llrs
from test_linkharq import SMALL, small_case
from test_linksim_gpu import _dev, _pinned

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEFAULT = ChannelSimConfig()
#: the frames of a case's batch behind the rounds of each group, per Q
GROUPS = {1: [[0], [1], [2], [3], [4]], 2: [[0, 1], [2, 0], [3, 3], [4, 1], [1, 4]], 3: [[0, 1, 2], [3, 4, 0], [4, 4, 4], [1, 0, 1]],
          4: [[0, 1, 2, 3], [4, 0, 1, 2], [3, 3, 3, 3], [2, 4, 4, 0]]}


def grouped(harq: HarqConfig):
    """``(llr [G Q, S, T, m] on the device, keys uint64 [G Q])``: the case's five frames regrouped for ``harq.rounds``."""
    frames = np.array(GROUPS[harq.rounds]).reshape(-1)
    return case_llrs(harq.link.sim, harq.link.bits_per_symbol)[frames].contiguous(), KEYS[frames]


def _harq_poisoned(harq: HarqConfig, llr: torch.Tensor, keys: torch.Tensor, want_bits=True, lib=None):
    """The entry point itself on outputs filled with values no decoder writes."""
    lib = lib or _lib.load()
    code, groups = harq.code, llr.shape[0] // harq.rounds
    counts = torch.full((groups, 7), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((groups, harq.blocks, harq.info_bits), 0xAB, dtype=torch.uint8, device=DEV)
    shifts = np.ascontiguousarray(code.shifts, dtype=np.int32)
    starts = np.ascontiguousarray(harq.starts, dtype=np.int32)
    _lib.check(lib.aft_link_harq_f32(ctypes.byref(harq.link.to_struct()), llr.data_ptr(), keys.data_ptr(), code.base_rows, code.base_cols,
                                     shifts.ctypes.data, harq.tx_cols, harq.rounds, starts.ctypes.data, harq.stride, harq.stride_inverse,
                                     code.qgain, code.offset, code.max_iters, counts.data_ptr(), bits.data_ptr() if want_bits else None,
                                     llr.shape[0], _lib.current_stream_ptr(llr.device)), lib)
    return counts, bits


def _equal_to_the_host(harq: HarqConfig, llr: torch.Tensor = None, keys: np.ndarray = None, lib=None):
    if llr is None:
        llr, keys = grouped(harq)
    want_counts, want_bits = link_harq_host(harq, keys, llr.cpu().numpy())
    counts, bits = _harq_poisoned(harq, llr, _dev(keys), lib=lib)
    assert bits.max().item() <= 1                                                # every element was written
    assert counts.cpu().tolist() == want_counts.tolist(), (harq.code.rate, harq.tx_cols, harq.rounds, harq.starts)
    assert torch.equal(bits.cpu(), torch.from_numpy(want_bits))
    bare, untouched = _harq_poisoned(harq, llr, _dev(keys), want_bits=False, lib=lib)      # bits = NULL: the same counts
    assert torch.equal(bare, counts) and (untouched == 0xAB).all()
    assert (want_counts[:, :4].sum(axis=1) + want_counts[:, 5] == harq.blocks).all()
    return want_counts


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0]}-{c[6]}")
def test_the_small_cases_of_the_host_tests(case):
    harq = small_case(*case)
    counts = _equal_to_the_host(harq)
    zeros = GROUPS[4].index([3, 3, 3, 3])
    assert counts[zeros, :4].sum() == 0 and counts[zeros, 6] == 4 * harq.blocks   # a group of zeros: one iteration per attempt, never acknowledged


@pytest.mark.parametrize("Q", (1, 2, 3, 4))
@pytest.mark.parametrize("mode", ("ir", "chase"))
def test_every_number_of_rounds_at_256_qam(Q, mode):
    harq = small_case("odd_30x7", 8, (4, 8), 5, Q, None, mode)
    assert (harq.blocks, harq.tx_bits, harq.used_bits) == (4, 320, 1280) and harq.link.bits_per_frame == 1560
    counts = _equal_to_the_host(harq)
    assert (counts[:, Q:4] == 0).all()


def test_more_blocks_than_waves():
    harq = HarqConfig(LdpcConfig(LinkConfig(DEFAULT, 8), (3, 4)), 2, 4)
    assert harq.blocks == 103                                                    # 16 waves: six full turns and one of seven
    _equal_to_the_host(harq)


def test_the_most_edges_share_the_lds_between_fewer_waves():
    """160 entries and n = 2048: 8 KiB of soft buffer and posteriors and 10 KiB of messages per block, so eight blocks in flight."""
    table = np.full((16, 16), -1, np.int32)
    rng = np.random.default_rng(2)
    table[:8, :] = rng.integers(0, 64, (8, 16))
    table[7, 0] = -1
    code = LdpcConfig(LinkConfig(ChannelSimConfig(ofdm=(240, 14)), 8), (16, 32), shifts=table, max_iters=4)
    harq = HarqConfig(code, 20, 2)
    assert code.edges == 160 and harq.blocks == 20 and harq.starts == (0, 20)     # the second window wraps
    assert (150 * 1024) // (2 * 2 * 2048 + 64 * 160) == 8 < harq.blocks
    _equal_to_the_host(harq)


def test_whole_codewords_given_starts_and_given_strides():
    whole = small_case("odd_30x7", 8, (3, 4), 4, 3, None, "ir")                  # C = nb: every round is the whole codeword
    assert whole.starts == (0, 0, 0)
    _equal_to_the_host(whole)
    _equal_to_the_host(small_case("odd_30x7", 8, (3, 4), 4, 3, (1, 3, 2), "ir"))
    _equal_to_the_host(small_case("edges_24x6", 6, (4, 6), 3, 4, (5, 5, 0, 3), "ir", offset=0, max_iters=7))
    for stride in (1, 383, 5):
        _equal_to_the_host(HarqConfig(LdpcConfig(LinkConfig(SIMS["odd_30x7"], 2), (3, 4)), 2, 2, stride=stride))
    _equal_to_the_host(HarqConfig(LdpcConfig(LinkConfig(DEFAULT, 6), "2/3"), 17, 2, stride=9791))      # U = 9792


def test_one_round_of_the_whole_codeword_is_the_ldpc_plan():
    for sim, m, rate in ((SIMS["odd_30x7"], 8, (4, 6)), (DEFAULT, 4, "1/2"), (DEFAULT, 8, (3, 4))):
        code = LdpcConfig(LinkConfig(sim, m), rate)
        harq = HarqConfig(code, code.base_cols, 1, stride=code.stride)
        llr, keys = grouped(harq)
        want, want_bits = LinkLdpcPlan(code, DEV)(llr, _dev(keys), want_bits=True)
        counts, bits = LinkHarqPlan(harq, DEV)(llr, _dev(keys), want_bits=True)
        assert torch.equal(bits, want_bits) and torch.equal(counts[:, 4:], want) and (counts[:, 1:4] == 0).all()
        assert torch.equal(counts[:, 0], code.blocks - want[:, 1])


def test_a_group_does_not_depend_on_its_batch_its_position_or_the_run():
    harq = small_case("odd_30x7", 8, (4, 8), 5, 3, None, "ir")
    plan = LinkHarqPlan(harq, DEV)
    five = case_llrs(harq.link.sim, 8)
    groups = GROUPS[3]
    order = [2, 0, 3, 3, 1, 0]
    frames = np.array([groups[g] for g in order]).reshape(-1)
    llr, keys = five[frames].contiguous(), _dev(KEYS[frames])
    counts, bits = plan(llr, keys, want_bits=True)
    assert counts.shape == (6, 7) and counts.dtype == torch.int32 and bits.shape == (6, 4, 256) and bits.dtype == torch.uint8
    alone = [plan(five[g].contiguous(), _dev(KEYS[g]), want_bits=True) for g in groups]
    for at, g in enumerate(order):
        assert torch.equal(counts[at:at + 1], alone[g][0]) and torch.equal(bits[at:at + 1], alone[g][1])
    again = plan(llr, keys, want_bits=True)
    assert torch.equal(again[0], counts) and torch.equal(again[1], bits)
    bare, none = plan(llr, keys)
    assert none is None and torch.equal(bare, counts)


def test_keys_in_pinned_memory_and_what_the_plan_refuses():
    harq = small_case("edges_24x6", 6, (3, 4), 3, 2, None, "ir")
    plan = LinkHarqPlan(harq, DEV)
    llr, keys = grouped(harq)
    want = plan(llr, _dev(keys), want_bits=True)
    got = plan(llr, _pinned(keys).reshape(-1, 1), want_bits=True)                # read in place
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    host = link_harq_host(harq, keys, llr.cpu().numpy())
    assert want[0].cpu().tolist() == host[0].tolist() and torch.equal(want[1].cpu(), torch.from_numpy(host[1]))
    kd = _dev(keys)
    for args, word in (((llr, torch.from_numpy(keys.view(np.int64).copy())), "pinned host memory"), ((llr, kd[:3]), "one value per frame"),
                       ((llr, kd.to(torch.int32)), "keys must be torch.int64"), ((llr.double(), kd), "llr must be float32"),
                       ((llr[:, :, :3], kd), "Expected llr shape"), ((llr[:0], kd[:0]), "Expected llr shape"),
                       ((llr[:5], kd[:5]), "not a multiple of rounds = 2"), ((llr.cpu(), kd), "must live on")):
        with pytest.raises(ValueError, match=word):
            plan(*args)
    with pytest.raises(ValueError, match="LinkHarqPlan runs on a HIP device"):
        LinkHarqPlan(harq, "cpu")
    with pytest.raises(ValueError, match="LinkHarqPlan needs a linksim.HarqConfig"):
        LinkHarqPlan(harq.code, DEV)


def test_every_refusal_of_the_entry_point_launches_nothing():
    harq = small_case("odd_30x7", 4, (3, 5), 3, 2, None, "ir")                   # kb = 2, E = 192, B = 4, U = 768 of 780 bits
    code = harq.code
    assert (harq.tx_bits, harq.blocks, harq.used_bits, harq.info_bits, harq.starts) == (192, 4, 768, 128, (0, 3))
    lib = _lib.load()
    llr, host_keys = grouped(harq)
    keys = _dev(host_keys)
    batch = llr.shape[0]
    counts = torch.full((batch // 2, 7), -7, dtype=torch.int32, device=DEV)
    bits = torch.full((batch // 2, 4, 128), 0xAB, dtype=torch.uint8, device=DEV)
    table = np.ascontiguousarray(code.shifts, dtype=np.int32)
    starts = np.ascontiguousarray(harq.starts, dtype=np.int32)
    good = dict(llr=llr.data_ptr(), keys=keys.data_ptr(), base_rows=3, base_cols=5, shifts=table.ctypes.data, tx_cols=3, rounds=2,
                starts=starts.ctypes.data, stride=harq.stride, stride_inverse=harq.stride_inverse, qgain=8.0, offset=4, max_iters=20,
                counts=counts.data_ptr(), bits=bits.data_ptr(), batch=batch)

    def call(p=None, **kw):
        a = dict(good, **kw)
        p = harq.link.to_struct() if p is None else p
        return lib.aft_link_harq_f32(ctypes.byref(p), *(a[n] for n in good), None)

    def refused(rc_want, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == rc_want and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error(), kw)

    def with_table(rows, cols, values, **more):
        t = np.ascontiguousarray(values, dtype=np.int32).reshape(rows, cols - rows)
        return dict(base_rows=rows, base_cols=cols, shifts=t.ctypes.data, **more), t      # the array is held by the caller

    def with_starts(values):
        s = np.ascontiguousarray(values, dtype=np.int32)
        return dict(starts=s.ctypes.data), s

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    assert lib.aft_link_harq_f32(None, *good.values(), None) == E and "NULL pointer" in lib.aft_last_error().decode()
    for name in ("llr", "keys", "shifts", "starts", "counts"):
        refused(E, "NULL pointer", **{name: None})
    refused(E, "8-byte", keys=good["keys"] + 4)
    for name in ("llr", "shifts", "starts", "counts"):
        refused(E, "4-byte", **{name: good[name] + 2})
    for b in (0, -2):
        refused(E, "batch must be at least 1", batch=b)
    for qgain in (0.0, -8.0, float("inf"), float("nan")):
        refused(E, "finite and positive", qgain=qgain)
    for b in (batch - 1, 1):
        refused(E, f"batch = {b} is not a multiple of rounds = 2", batch=b)
    for rounds in (0, 5, -1):
        refused(SH, f"rounds = {rounds} is outside 1..4", rounds=rounds)
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
    kw, held = with_table(16, 32, dense, tx_cols=17)
    refused(SH, "161 entries", **kw)
    for C_ in (2, 0, 6, -1):
        refused(SH, f"tx_cols = {C_} is outside 3..5", tx_cols=C_)
    for values, at in (([0, 5], 1), ([-1, 0], 0), ([1 << 20, 0], 0)):
        kw, held = with_starts(values)
        refused(SH, f"starts[{at}] = {values[at]} is outside 0..4", **kw)
    kw, held = with_table(3, 16, np.zeros((3, 13), np.int32), tx_cols=14)
    refused(SH, "fewer than the 896 coded bits", **kw)                           # 780 bits per frame
    for stride in (0, 768, 769, 1 << 40):
        refused(SH, "is outside [1, 768)", stride=stride)
    for stride in (2, 3, 384):
        refused(SH, "not coprime", stride=stride)
    for inverse in (0, 768, harq.stride_inverse + 1, 1):
        refused(SH, "is not the inverse", stride_inverse=inverse)
    many = harq.link.to_struct()
    many.num_scs, many.num_symbols = 1 << 16, 1 << 15                            # 2^31 elements of 16-QAM: 2^26 blocks of 128 bits
    refused(SH, "more than 2^31", p=many)

    def struct(**fields):
        p = harq.link.to_struct()
        for name, value in fields.items():
            setattr(p, name, value)
        return p

    for fields, word in ((dict(num_scs=0), "num_scs = 0"), (dict(num_symbols=-1), "num_symbols = -1"),
                         (dict(num_scs=1 << 16, num_symbols=(1 << 15) + 1), "more than 2^31 elements"),
                         (dict(pilot_scs=65), "pilot_scs = 65 is outside 1..64"), (dict(pilot_symbols=0), "pilot_symbols = 0"),
                         (dict(num_symbols=2), "larger than the ofdm grid"), (dict(bits_per_symbol=3), "bits_per_symbol = 3")):
        refused(SH, word, p=struct(**fields))
    torch.cuda.synchronize()
    assert (counts == -7).all() and (bits == 0xAB).all()                         # nothing was launched
    assert call() == _abi.AFT_OK and call(bits=None) == _abi.AFT_OK              # a NULL bits is legal
    torch.cuda.synchronize()
    want_counts, want_bits = link_harq_host(harq, host_keys, llr.cpu().numpy())
    assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_link_harq_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_link_harq_f32")
    for case in SMALL:
        _equal_to_the_host(small_case(*case), lib=lib)
    _equal_to_the_host(small_case("odd_30x7", 8, (4, 8), 5, 3, None, "ir"), lib=lib)
    _equal_to_the_host(HarqConfig(LdpcConfig(LinkConfig(DEFAULT, 8), (3, 4)), 2, 2), lib=lib)
    _equal_to_the_host(HarqConfig(LdpcConfig(LinkConfig(DEFAULT, 2), (16, 32)), 17, 2), lib=lib)


@pytest.mark.parametrize("value", (float("nan"), 1e30, float("-inf")))
def test_the_bits_do_not_depend_on_what_the_lds_held(value):
    for harq in (small_case("odd_30x7", 8, (4, 8), 5, 4, None, "ir"), HarqConfig(LdpcConfig(LinkConfig(DEFAULT, 4), "1/2"), 16, 2),
                 HarqConfig(LdpcConfig(LinkConfig(DEFAULT, 8), (3, 4)), 2, 2)):
        plan = LinkHarqPlan(harq, DEV)
        llr, keys = grouped(harq)
        want = plan(llr, _dev(keys), want_bits=True)
        fill_lds(value, "cuda:0")
        got = plan(llr, _dev(keys), want_bits=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    host = link_harq_host(harq, keys, llr.cpu().numpy())
    assert got[0].cpu().tolist() == host[0].tolist() and torch.equal(got[1].cpu(), torch.from_numpy(host[1]))


def test_physical_sanity_on_the_device():
    """12 dB, 16-QAM, mother code 1/2, 16 of 24 columns per round: perfect channel knowledge delivers every block, the LS estimate
    does not, and both equal the host twin on the device's own LLRs."""
    from test_linkharq import harq_sanity_inputs
    code, keys, sigma, scale, ideal, est = harq_sanity_inputs()
    harq = HarqConfig(code, 16, 4)
    soft, plan = LinkSoftPlan(code.link, DEV), LinkHarqPlan(harq, DEV)
    total = {}
    for which, e in est.items():
        _, llr = soft(_dev(ideal), _dev(e), _dev(keys), _dev(sigma), _dev(scale), torch.ones(1, device=DEV), want_llr=True)
        counts, bits = plan(llr, _dev(keys), want_bits=True)
        want_counts, want_bits = link_harq_host(harq, keys, llr.cpu().numpy())
        assert counts.cpu().tolist() == want_counts.tolist() and torch.equal(bits.cpu(), torch.from_numpy(want_bits))
        total[which] = counts.sum(dim=0).tolist()
    print("counts of 24 blocks:", total)
    assert total["ideal"][5] == 0 and total["ls"][5] >= 1 and sum(total["ideal"][:2]) > sum(total["ls"][:2])


def test_harq_accumulator_runs_from_the_loader_without_a_synchronisation():
    sim = ChannelSimConfig()
    harq = HarqConfig(LdpcConfig(LinkConfig(sim, 4), "1/2"), 16, 4)
    model = LmmseEstimator(sim).to(DEV).eval()
    loader = SynthLoader(sim, 16, 16 * 3, device=DEV, seed=2)
    with_est, perfect, on_device, two = (HarqAccumulator(harq, DEV, seed=2, branches=b) for b in (1, 1, 1, 2))
    it = iter(loader)
    first = next(it)
    seen = []

    def step(batch):
        pil, ideal, meta = batch
        est = model(pil, meta)
        with_est.update(est, ideal, meta)
        perfect.update(None, ideal, meta)
        on_device.update(est, ideal, frame_ids=meta[0].to(DEV, non_blocking=True), snr_db=meta[1])
        two.update(est, ideal, meta)
        seen.append((ideal, est, meta))

    step(first)                                   # the first batch builds the plans and the pinned blocks: outside the guard
    torch.cuda.synchronize()
    probe = torch.ones((), device=DEV)
    with _no_sync():
        with pytest.raises(RuntimeError):
            probe.item()                          # the mode is honoured: what follows is not vacuous
        for batch in it:
            step(batch)
    assert len(seen) == 3 and with_est.frames == perfect.frames == 48 and two.frames == 24
    assert with_est.errors.is_cuda and with_est.errors.dtype == torch.int64 and with_est.errors.shape == (7,)
    # what the accumulator launched, step by step: the soft plan's LLRs through the host twin
    soft = LinkSoftPlan(harq.link, DEV)
    want = np.zeros((2, 7), np.int64)
    for ideal, est, meta in seen:
        g = np.rint(meta[0].numpy().reshape(-1)).astype(np.int64)
        snr = meta[1].numpy().reshape(-1)
        keys = frame_keys(2, g)
        for i, e in enumerate((est, ideal)):
            _, llr = soft(ideal, e, _dev(keys), _dev(noise_sigma(snr)), _dev(llr_scale(snr)), torch.ones(1, device=DEV), want_llr=True)
            want[i] += link_harq_host(harq, keys, llr.cpu().numpy())[0].sum(axis=0)
    assert with_est.errors.cpu().tolist() == want[0].tolist() and perfect.errors.cpu().tolist() == want[1].tolist()
    assert on_device.errors.cpu().tolist() == with_est.errors.cpu().tolist()
    blocks = 12 * harq.blocks
    acked, failed = want[0][:4], want[0][5]
    used = int((acked * np.arange(1, 5)).sum() + 4 * failed)
    assert acked.sum() + failed == blocks and int(two.errors[:4].sum() + two.errors[5]) == 6 * harq.blocks
    assert with_est.result() == failed / blocks and with_est.result_transmissions() == used / blocks
    assert with_est.result_bler_after(1) == (blocks - acked[:2].sum()) / blocks and with_est.result_iterations() == want[0][6] / blocks
    assert with_est.result_throughput() == harq.info_bits * int(acked.sum()) * harq.blocks / (harq.link.data_elements * used)
    print(f"throughput with the LMMSE estimate {with_est.result_throughput():.3f}, with the channel {perfect.result_throughput():.3f}, "
          f"two antennas {two.result_throughput():.3f}; rounds {with_est.result_transmissions():.2f}, {perfect.result_transmissions():.2f}, "
          f"{two.result_transmissions():.2f}")


def test_harq_sweep_over_simulated_packs_equals_the_host_twin_on_the_devices_llrs():
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import make_pack
    from adafortitran_amd.evaluation import get_link_harq
    sim = ChannelSimConfig()
    harq = HarqConfig(LdpcConfig(LinkConfig(sim, 4), "1/2"), 16, 4)
    packs = {snr: make_pack(sim, 16, seed=20 + snr, snr_db=snr) for snr in (5, 25)}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(pack, sim.pilot, 8, device=DEV, shuffle=False)) for snr, pack in packs.items()]
    got = get_link_harq(None, loaders, harq, seed=1)
    soft = LinkSoftPlan(harq.link, DEV)
    want = {}
    for name, loader in loaders:
        snr_key = int(name.split("_")[1])
        counts = np.zeros(7, np.int64)
        for _, ideal, meta in loader:
            g = np.rint(meta[0].cpu().numpy().reshape(-1)).astype(np.int64)
            snr = meta[1].cpu().numpy().reshape(-1)
            keys = frame_keys(1, g)
            _, llr = soft(ideal, ideal, _dev(keys), _dev(noise_sigma(snr)), _dev(llr_scale(snr)), torch.ones(1, device=DEV), want_llr=True)
            counts += link_harq_host(harq, keys, llr.cpu().numpy())[0].sum(axis=0)
        acked = counts[:4]
        used = int((acked * np.arange(1, 5)).sum() + 4 * counts[5])
        want[snr_key] = harq.info_bits * int(acked.sum()) * harq.blocks / (harq.link.data_elements * used)
    print("throughput with the channel", got)
    assert list(got) == [5, 25] and got == want and 0 <= got[5] < got[25]
