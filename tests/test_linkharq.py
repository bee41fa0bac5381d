"""The HARQ link of ``adafortitran_amd.linksim`` on the CPU: the identity with the LDPC-coded link at one round of the whole codeword,
``link_harq_host`` against a second evaluation written with plain loops (rate matcher, positions, soft buffer) around the scalar
row-by-row decoder of tests/test_linkldpc.py, its fixed points (noiseless LLRs, a frame of zeros), what has no influence, every
refusal of ``HarqConfig``, ``HarqAccumulator``'s results against hand arithmetic, the binding's new names and the physical sanity
figures.  Everything is compared for equality.

tests/test_linkharq_gpu.py compares the kernel with ``link_harq_host``."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi
from adafortitran_amd.chansim import STREAM_CODE_BITS, ChannelSimConfig, frame_keys, ls_interpolate, simulate_frames_host, words
from adafortitran_amd.linksim import (HARQ_COUNTS, HARQ_MAX_ROUNDS, HarqAccumulator, HarqConfig, LdpcBlockErrorAccumulator, LdpcConfig,
                                      LinkConfig, default_stride, ldpc_encode, link_harq_host, link_ldpc_host, link_llrs_host, llr_scale,
                                      noise_sigma, quantise)
from test_linkcode import SEED, SIMS, noiseless_llrs, sent_words_bits
from test_linkldpc import scalar_decode

#: the two small cases of the issue: (grid, m, mother code, C, Q, starts or None, mode)
SMALL = (("odd_30x7", 2, (3, 4), 2, 4, None, "ir"), ("odd_30x7", 2, (3, 4), 2, 4, None, "chase"),
         ("edges_24x6", 4, (4, 8), 5, 4, (0, 5, 2, 7), "ir"))


def small_case(name, m, rate, C, Q, starts, mode, **kw) -> HarqConfig:
    return HarqConfig(LdpcConfig(LinkConfig(SIMS[name], m), rate, **kw), C, Q, starts=starts, mode=mode)


def noisy_llrs(harq: HarqConfig, keys, rng, noise: float) -> np.ndarray:
    """Each frame's own sent words as LLRs of magnitude 1, plus Gaussian noise: blocks decode after different numbers of rounds."""
    clean = noiseless_llrs(harq, keys, 1.0)
    return (clean + rng.normal(0.0, noise, clean.shape)).astype(np.float32)


def info_bits(harq: HarqConfig, leaders) -> np.ndarray:
    """uint8 ``[G, B, K]``: stream 8 of the leaders' keys."""
    B, K = harq.blocks, harq.info_bits
    index = np.arange(B * K, dtype=np.uint64).reshape(1, B, K)
    return (words(np.asarray(leaders)[:, None, None], STREAM_CODE_BITS, index) >> np.uint64(63)).astype(np.uint8)


def loops_harq(harq: HarqConfig, keys, llr):
    """The definition with plain loops: one transmitted bit at a time into the soft buffer, then the scalar decoder."""
    code, link, Q, C = harq.code, harq.link, harq.rounds, harq.tx_cols
    (S, T), m, nb, K, n = link.sim.ofdm, link.bits_per_symbol, code.base_cols, code.info_bits, code.coded_bits
    E = 64 * C
    B = link.bits_per_frame // E
    U, A = B * E, harq.stride
    data = [q for q in range(S * T) if link.data_mask.reshape(-1)[q]]             # the grid elements that are no pilot, row-major
    sent_bits = sent_words_bits(link, keys)                                        # [frames, S, T, m]
    G = len(keys) // Q
    counts = np.zeros((G, 7), np.int64)
    bits = np.zeros((G, B, K), np.uint8)
    for h in range(G):
        u = info_bits(harq, keys[h * Q:h * Q + 1])[0]
        for b in range(B):
            c = ldpc_encode(code, u[b])
            Z = [0] * n
            acked = False
            for t in range(Q):
                f = h * Q + t
                for e in range(E):
                    v = 64 * ((harq.starts[t] + e // 64) % nb) + e % 64
                    j = ((b * E + e) * A) % U
                    q, k = data[j // m], j % m
                    s = int(sent_bits[f, q // T, q % T, k]) ^ int(c[v])
                    lam = llr[f, q // T, q % T, k]
                    Z[v] += int(quantise(np.float32(-lam if s else lam), code.qgain))
                got, it = scalar_decode(code, Z)
                counts[h, 6] += it
                bits[h, b] = got
                if (got == u[b]).all():
                    counts[h, t] += 1
                    acked = True
                    break
            if not acked:
                counts[h, 4] += int((bits[h, b] != u[b]).sum())
                counts[h, 5] += 1
    return counts, bits


def test_one_round_of_the_whole_codeword_is_the_ldpc_coded_link():
    rng = np.random.default_rng(1)
    keys = frame_keys(SEED, np.arange(3))
    for name, m, rate, kw in (("odd_30x7", 8, (3, 4), {}), ("edges_24x6", 6, (4, 6), dict(stride=7)), ("odd_30x7", 4, (3, 5), dict(max_iters=5)),
                              (None, 4, "1/2", {})):
        code = LdpcConfig(LinkConfig(ChannelSimConfig() if name is None else SIMS[name], m), rate, **kw)
        harq = HarqConfig(code, code.base_cols, 1, stride=code.stride)
        assert harq.starts == (0,) and (harq.blocks, harq.used_bits, harq.tx_bits) == (code.blocks, code.used_bits, code.coded_bits)
        assert HarqConfig(code, code.base_cols, 1).stride == default_stride(code.used_bits)      # the same golden section
        assert (harq.positions() == code.positions()).all()
        llr = noisy_llrs(harq, keys, rng, 0.9)
        counts, bits = link_harq_host(harq, keys, llr)
        want, want_bits = link_ldpc_host(code, keys, llr)
        assert counts.dtype == np.int64 and counts.shape == (3, 7) and bits.dtype == np.uint8
        assert (bits == want_bits).all()
        assert counts[:, 0].tolist() == (code.blocks - want[:, 1]).tolist() and (counts[:, 1:4] == 0).all()
        assert counts[:, 4:].tolist() == want.tolist()
        assert 0 < want[:, 1].sum() or name is None


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0]}-{c[6]}")
def test_the_host_twin_equals_plain_loops_around_the_scalar_decoder(case):
    harq = small_case(*case, max_iters=6)
    Q = harq.rounds
    if case[0] == "odd_30x7":
        assert (harq.blocks, harq.tx_bits, harq.used_bits) == (3, 128, 384) and harq.starts == ((0, 2, 0, 2) if case[6] == "ir" else (0,) * 4)
    else:
        assert (harq.blocks, harq.tx_bits, harq.used_bits) == (1, 320, 320) and harq.starts == (0, 5, 2, 7)
        assert set(harq.windows()[1] // 64) == {5, 6, 7, 0, 1}                     # the window wraps past column nb - 1 inside a round
    keys = frame_keys(SEED, np.arange(3 * Q))
    llr = noisy_llrs(harq, keys, np.random.default_rng(4), 1.1)
    llr[2 * Q:] = (np.random.default_rng(5).integers(-4, 5, llr[2 * Q:].shape) / 8.0).astype(np.float32)      # ties and garbage
    counts, bits = link_harq_host(harq, keys, llr)
    want_counts, want_bits = loops_harq(harq, keys, llr)
    print(case, counts.tolist())
    assert counts.tolist() == want_counts.tolist() and (bits == want_bits).all()
    assert counts[:, :4].sum() > 0 and counts[:, 5].sum() > 0                      # some blocks are delivered, some never
    assert (counts[:, :4].sum(axis=1) + counts[:, 5] == harq.blocks).all()


def test_the_windows_and_the_positions():
    harq = small_case("edges_24x6", 4, (4, 8), 5, 4, (0, 5, 2, 7), "ir")
    v = harq.windows()
    assert v.shape == (4, 320) and v.dtype == np.int64
    assert v[0].tolist() == list(range(320)) and v[1][:64].tolist() == list(range(320, 384)) and v[1][192:256].tolist() == list(range(64))
    assert all(len(set(row.tolist())) == 320 for row in v)                        # a round holds every variable at most once
    ir = small_case("odd_30x7", 8, (4, 8), 5, 4, None, "ir")
    assert ir.starts == (0, 5, 2, 7) and small_case("odd_30x7", 8, (4, 8), 5, 3, None, "chase").starts == (0, 0, 0)
    assert sorted(ir.positions().reshape(-1).tolist()) == list(range(ir.used_bits)) and ir.positions().shape == (ir.blocks, 320)
    assert ir.stride == default_stride(ir.used_bits) and (ir.stride * ir.stride_inverse) % ir.used_bits == 1
    assert ir.info_bits_per_frame == ir.blocks * 256 and ir.link is ir.code.link


@pytest.mark.parametrize("mode", ("ir", "chase"))
def test_noiseless_llrs_are_acknowledged_at_round_0(mode):
    for name, m, rate, C, Q in (("odd_30x7", 2, (3, 4), 2, 4), ("edges_24x6", 4, (4, 8), 5, 3), ("odd_30x7", 8, (4, 6), 3, 2)):
        harq = small_case(name, m, rate, C, Q, None, mode)
        keys = frame_keys(SEED, np.arange(2 * Q))
        counts, bits = link_harq_host(harq, keys, noiseless_llrs(harq, keys))
        assert counts[:, 0].tolist() == [harq.blocks] * 2 and (counts[:, 1:6] == 0).all()
        assert (bits == info_bits(harq, keys[::Q])).all()
        assert (counts[:, 6] >= harq.blocks).all()


@pytest.mark.parametrize("poison", (np.nan, 1e30, -np.inf))
def test_what_has_no_influence(poison):
    """The later rounds' LLRs of acknowledged blocks, the filler and the pilots."""
    for case in SMALL[1:]:
        harq = small_case(*case)
        Q, m = harq.rounds, harq.link.bits_per_symbol
        S, T = harq.link.sim.ofdm
        keys = frame_keys(SEED, np.arange(3 * Q))
        llr = noisy_llrs(harq, keys, np.random.default_rng(9), 1.0)
        want = link_harq_host(harq, keys, llr)
        info = info_bits(harq, keys[::Q])
        last = np.full((3, harq.blocks), Q - 1)                                   # the last round a block's attempt ran after
        for upto in range(Q - 1, 0, -1):                                          # the same link cut short after `upto` rounds
            short = HarqConfig(harq.code, harq.tx_cols, upto, starts=harq.starts[:upto], stride=harq.stride)
            frames = np.concatenate([np.arange(h * Q, h * Q + upto) for h in range(3)])
            got = link_harq_host(short, keys[frames], llr[frames])[1]
            last[(got == info).all(axis=-1)] = upto - 1
        assert (last < Q - 1).any() and want[0][:, :Q - 1].sum() == (last < Q - 1).sum()
        used = np.zeros((3 * Q, S * T * m), bool)
        j = harq.positions()
        at = np.flatnonzero(harq.link.data_mask)[j // m] * m + j % m               # [B, E]
        for h in range(3):
            for b in range(harq.blocks):
                for t in range(last[h, b] + 1):
                    used[h * Q + t, at[b]] = True
        assert not used.reshape(-1, S, T, m)[:, ~harq.link.data_mask].any() and not used.all(axis=1).any()
        bad = llr.copy().reshape(3 * Q, -1)
        bad[~used] = poison
        got = link_harq_host(harq, keys, bad.reshape(llr.shape))
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_a_group_of_zeros_is_never_acknowledged():
    harq = small_case("odd_30x7", 8, (3, 4), 2, 4, None, "ir")
    keys = frame_keys(SEED, np.arange(8))
    llr = noiseless_llrs(harq, keys)
    llr[4:] = 0.0                                                                # the second group: every input quantises to 0
    counts, bits = link_harq_host(harq, keys, llr)
    info = info_bits(harq, keys[::4])
    assert info[1].any(axis=-1).all()                                            # no block's u is all-zero
    B = harq.blocks
    assert counts[0].tolist()[:6] == [B, 0, 0, 0, 0, 0]
    assert counts[1].tolist() == [0, 0, 0, 0, int(info[1].sum()), B, 4 * B]       # the zero word satisfies every check after one iteration
    assert not bits[1].any() and (bits[0] == info[0]).all()


def test_harq_config_validates():
    link = LinkConfig(SIMS["odd_30x7"], 2)                                       # 390 bits per frame
    code = LdpcConfig(link, (3, 5))                                              # kb = 2, n = 320
    harq = HarqConfig(code, 3)
    assert (harq.rounds, harq.mode, harq.starts, harq.tx_bits, harq.blocks, harq.used_bits) == (4, "ir", (0, 3, 1, 4), 192, 2, 384)
    assert HARQ_MAX_ROUNDS == 4 and HARQ_COUNTS == 7
    with pytest.raises(ValueError, match="needs an LdpcConfig"):
        HarqConfig(link, 3)
    for C_ in (2, 0, 6, -1, 3.0, True, None):
        with pytest.raises(ValueError, match=re.escape("tx_cols = ") + ".*an integer in 3 .. 5"):
            HarqConfig(code, C_)
    for Q in (0, 5, -1, 2.0, False):
        with pytest.raises(ValueError, match="rounds = .*an integer in 1 .. 4"):
            HarqConfig(code, 3, Q)
    with pytest.raises(ValueError, match="mode = 'both'"):
        HarqConfig(code, 3, mode="both")
    for starts in ((0, 1, 2), (0, 1, 2, 3, 4), 7):
        with pytest.raises(ValueError, match="4 block columns, one per round"):
            HarqConfig(code, 3, starts=starts)
    for starts in ((0, 1, 2, 5), (0, -1, 2, 3), (0, 1.0, 2, 3), (0, True, 2, 3)):
        with pytest.raises(ValueError, match="every start is a block column in 0 .. 4"):
            HarqConfig(code, 3, starts=starts)
    assert HarqConfig(code, 3, 2, starts=[4, np.int64(0)]).starts == (4, 0)
    for stride in (0, 384, -5, 2.5, True):
        with pytest.raises(ValueError, match=re.escape("an integer in [1, 384)")):
            HarqConfig(code, 3, stride=stride)
    for stride in (2, 3, 192):
        with pytest.raises(ValueError, match="not coprime to the 384 used bits"):
            HarqConfig(code, 3, stride=stride)
    assert HarqConfig(code, 3, stride=383).stride_inverse == 383
    with pytest.raises(ValueError, match="fewer than the 1536 coded bits"):        # the mother code itself must fit the link
        HarqConfig(LdpcConfig(link, "1/2"), 13)
    with pytest.raises(Exception):
        harq.rounds = 2                                                          # frozen
    keys = frame_keys(SEED, np.arange(4))
    with pytest.raises(ValueError, match="needs a HarqConfig"):
        link_harq_host(code, keys, np.zeros((4, 30, 7, 2), np.float32))
    with pytest.raises(ValueError, match="not a positive multiple of rounds = 4"):
        link_harq_host(harq, keys[:3], np.zeros((3, 30, 7, 2), np.float32))
    with pytest.raises(ValueError, match="Expected llr of shape"):
        link_harq_host(harq, keys, np.zeros((4, 30, 7, 4), np.float32))


def test_the_accumulator_against_hand_arithmetic():
    link = LinkConfig(SIMS["odd_30x7"], 8)                                       # 195 data elements, 1560 bits
    harq = HarqConfig(LdpcConfig(link, (3, 4)), 2, 4)                            # K = 64, E = 128: B = 12
    assert harq.blocks == 12 and link.data_elements == 195
    acc = HarqAccumulator(harq, "cpu")
    assert acc.errors.shape == (7,) and acc.errors.dtype == torch.int64 and acc.frames == 0
    for empty in (acc.result(), acc.result_bler_after(0), acc.result_transmissions(), acc.result_throughput(), acc.result_iterations(),
                  acc.result_ber()):
        assert empty == 0.0
    acc.errors += torch.tensor([5, 10, 3, 2, 77, 4, 333])                       # two groups: 24 blocks, 20 delivered
    acc.frames = 8
    assert acc.result() == 4 / 24
    assert [acc.result_bler_after(t) for t in range(4)] == [19 / 24, 9 / 24, 6 / 24, 4 / 24]
    used = 5 * 1 + 10 * 2 + 3 * 3 + 2 * 4 + 4 * 4                                # 58 block rounds
    assert acc.result_transmissions() == used / 24
    assert acc.result_throughput() == 64 * 20 * 12 / (195 * used)
    assert acc.result_iterations() == 333 / 24 and acc.result_ber() == 77 / (24 * 64)
    for t in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="a round in 0 .. 3"):
            acc.result_bler_after(t)
    with pytest.raises(ValueError, match="needs a HarqConfig"):
        HarqAccumulator(harq.code, "cpu")
    with pytest.raises(ValueError, match="not a multiple of branches \\* rounds = 2 \\* 4"):
        HarqAccumulator(harq, "cpu", branches=2).update(None, torch.zeros((12, 30, 7), dtype=torch.complex64), frame_ids=np.arange(12), snr_db=10.0)


def test_the_binding():
    assert _abi.AFT_ABI_VERSION == 10 and _abi.AFT_LINK_HARQ_MAX_ROUNDS == 4 and _abi.AFT_LINK_HARQ_COUNTS == 7
    restype, argtypes = _abi.SIGNATURES["aft_link_harq_f32"]
    assert "aft_link_harq_f32" in _abi.EXPORTED_SYMBOLS and restype is C.c_int and len(argtypes) == 18
    assert argtypes[0] is C.POINTER(_abi.AftLink) and argtypes[9] is argtypes[10] is C.c_ulonglong and argtypes[11] is C.c_float
    assert [argtypes[i] for i in (3, 4, 6, 7, 12, 13, 16)] == [C.c_int] * 7
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_harq_f32") == names.index("aft_link_mrc_f32") + 1 == names.index("aft_link_ldpc_f32") + 2


# ---- physical sanity: the default grid, 16-QAM, 12 dB, mother code 1/2, 16 of 24 columns per round, 4 rounds, seed 3, frames 0 .. 15 ----

_sanity = []
#: what link_harq_host returns, summed over the four groups
PINNED = {("ideal", "ir"): [0, 24, 0, 0, 0, 0, 541], ("ideal", "chase"): [0, 7, 17, 0, 0, 0, 982],
          ("ls", "ir"): [0, 7, 4, 0, 727, 13, 1436], ("ls", "chase"): [0, 0, 2, 4, 1297, 18, 1829]}


def harq_sanity_inputs():
    """(code, keys, sigma, scale, ideal, {"ideal": .., "ls": ..}) made once: 16 frames = 4 groups of 4 rounds, 6 blocks each."""
    if not _sanity:
        sim = ChannelSimConfig(snr_db=(12.0,))
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(16))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        code = LdpcConfig(LinkConfig(sim, 4), "1/2")
        _sanity.append((code, frame_keys(SEED, np.arange(16)), noise_sigma(meta[:, 0]), llr_scale(meta[:, 0]), ideal,
                        {"ideal": ideal, "ls": ls_interpolate(sim, pilots)}))
    return _sanity[0]


def test_physical_sanity_and_the_accumulator_on_the_host():
    code, keys, sigma, scale, ideal, est = harq_sanity_inputs()
    meta = (torch.arange(16, dtype=torch.float32).reshape(16, 1), torch.full((16, 1), 12.0))
    total = {}
    for which, e in est.items():
        llr = link_llrs_host(code.link, keys, ideal, e, sigma, scale)[1]
        for mode in ("ir", "chase"):
            harq = HarqConfig(code, 16, 4, mode=mode)
            assert harq.blocks * 4 == 24
            counts, _ = link_harq_host(harq, keys, llr)
            total[which, mode] = counts.sum(axis=0).tolist()
            acc = HarqAccumulator(harq, "cpu", seed=SEED)
            for lo, hi in ((0, 12), (12, 16)):                                    # two batches: three groups and one
                acc.update(None if which == "ideal" else torch.from_numpy(e[lo:hi]), torch.from_numpy(ideal[lo:hi]),
                           tuple(t[lo:hi] for t in meta))
            assert acc.frames == 16 and acc.errors.tolist() == total[which, mode]
    print(total)
    assert total["ideal", "ir"][5] == total["ideal", "chase"][5] == 0            # perfect knowledge leaves no block undelivered
    assert total["ls", "ir"][5] > 0 and total["ls", "chase"][5] > 0               # the LS estimate leaves some
    for which in est:
        assert sum(total[which, "ir"][:2]) >= sum(total[which, "chase"][:2])     # by round 1 new parity is worth more than a repeat
    assert total == PINNED
    a = total["ls", "ir"]
    used = 7 * 2 + 4 * 3 + 13 * 4
    assert acc.result() == 18 / 24                                               # the last one opened: LS, chase
    ir = HarqAccumulator(HarqConfig(code, 16, 4), "cpu", seed=SEED)
    ir.update(torch.from_numpy(est["ls"]), torch.from_numpy(ideal), meta)
    assert ir.errors.tolist() == a and ir.result() == 13 / 24 and ir.result_transmissions() == used / 24
    assert ir.result_throughput() == 768 * 11 * 6 / (code.link.data_elements * used)


def test_one_round_accumulates_what_the_ldpc_accumulator_does():
    code, keys, sigma, scale, ideal, est = harq_sanity_inputs()
    meta = (torch.arange(4, dtype=torch.float32).reshape(4, 1), torch.full((4, 1), 12.0))
    single = LdpcBlockErrorAccumulator(code, "cpu", seed=SEED)
    harq = HarqAccumulator(HarqConfig(code, 24, 1), "cpu", seed=SEED)
    for acc in (single, harq):
        acc.update(torch.from_numpy(est["ls"][:4]), torch.from_numpy(ideal[:4]), meta)
    bit_errors, block_errors, iterations = single.errors.tolist()
    assert harq.errors.tolist() == [16 - block_errors, 0, 0, 0, bit_errors, block_errors, iterations]
    assert harq.result() == single.result() and harq.result_throughput() == single.result_throughput()
    assert harq.result_iterations() == single.result_iterations() and harq.result_ber() == single.result_ber()
    assert harq.result_transmissions() == 1.0
