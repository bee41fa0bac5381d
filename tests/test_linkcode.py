"""The coded link of ``adafortitran_amd.linksim`` on the CPU: the code's known answer and sizes, the noiseless round trip, the host
decoder against a brute force over all inputs (largest metric and the tie rule), the interleaver, the quantiser's edges, filler and
pilot LLRs without influence, ``CodeConfig``'s refusals, the binding's new names, ``BlockErrorAccumulator`` / ``get_link_bler`` on the
host, and the physical sanity figures.

``code_case`` builds the small links tests/test_linkcode_gpu.py compares the kernel on; the GPU file imports it."""
import itertools
import math

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, chansim
from adafortitran_amd.chansim import ChannelSimConfig, frame_keys, ls_interpolate, make_pack, simulate_frames_host, words
from adafortitran_amd.linksim import (BITS_PER_SYMBOL, MAX_INFO_BITS, RATES, STREAM_CODE_BITS, STREAM_DATA_BITS, BlockErrorAccumulator,
                                      CodeConfig, LinkConfig, coded_bits, conv_encode, default_stride, keep_mask, link_decode_host,
                                      link_encode_host, link_llrs_host, llr_scale, noise_sigma, quantise, viterbi_host)

SEED = 3
# the small grids: odd T; pilots on the first and the last grid element; pilot rows that hold no data element at all
SIMS = {
    "odd_30x7": ChannelSimConfig(ofdm=(30, 7), pilot=(5, 3)),
    "edges_24x6": ChannelSimConfig(ofdm=(24, 6), pilot=(3, 2), pilot_scs=(0, 9, 23), pilot_symbols=(0, 5)),
    "full_rows_40x2": ChannelSimConfig(ofdm=(40, 2), pilot=(3, 2), pilot_scs=(0, 1, 39)),
    "small_12x4": ChannelSimConfig(ofdm=(12, 4), pilot=(4, 2)),
}


def sent_words_bits(cfg: LinkConfig, keys) -> np.ndarray:
    """uint8 ``[n, S, T, m]``: bit k of the sent word of every grid element, MSB first (the LLR tensor's last axis)."""
    S, T = cfg.sim.ofdm
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T, 1)
    shift = np.uint64(63) - np.arange(cfg.bits_per_symbol, dtype=np.uint64).reshape(1, 1, 1, -1)
    return ((words(np.asarray(keys)[:, None, None, None], STREAM_DATA_BITS, q) >> shift) & np.uint64(1)).astype(np.uint8)


def noiseless_llrs(code: CodeConfig, keys, c: float = 4.0) -> np.ndarray:
    """float32 ``[n, S, T, m]``: ``llr_j = (1 - 2 w_j) c``, the LLRs of a demapper that is right about every sent bit; descrambled they
    are ``(1 - 2 c_p) c``, the codeword's own signs."""
    cfg = code.link
    (S, T), m = cfg.sim.ofdm, cfg.bits_per_symbol
    w = sent_words_bits(cfg, keys)
    return ((1.0 - 2.0 * w) * c).astype(np.float32).reshape(len(keys), S, T, m)


def test_impulse_known_answer_and_weight():
    out = conv_encode(np.array([1]), "1/2").reshape(7, 2)
    assert out[:, 0].tolist() == [1, 0, 1, 1, 0, 1, 1] and out[:, 1].tolist() == [1, 1, 1, 1, 0, 0, 1] and out.sum() == 10
    out7 = conv_encode(np.array([1, 0, 0, 0, 0, 0, 0]), "1/2").reshape(13, 2)
    assert (out7[:7] == out).all() and out7[7:].sum() == 0
    assert conv_encode(np.zeros((3, 5), np.uint8), "3/4").sum() == 0


def _scalar_encode(u, rate):
    """An encoder written bit by bit, independent of conv_encode's slicing."""
    period = {"1/2": ["AB"], "2/3": ["AB", "A"], "3/4": ["AB", "A", "B"]}[rate]
    u = list(u) + [0] * 6
    at = lambda t: u[t] if t >= 0 else 0  # noqa: E731
    out = []
    for t in range(len(u)):
        a = at(t) ^ at(t - 2) ^ at(t - 3) ^ at(t - 5) ^ at(t - 6)
        b = at(t) ^ at(t - 1) ^ at(t - 2) ^ at(t - 3) ^ at(t - 6)
        out += [{"A": a, "B": b}[o] for o in period[t % len(period)]]
    return out


@pytest.mark.parametrize("rate", RATES)
def test_coded_bits_per_rate(rate):
    per = {"1/2": (1, [2]), "2/3": (2, [2, 1]), "3/4": (3, [2, 1, 1])}[rate]
    for K in (1, 2, 3, 511, 512, 513):
        want = sum(per[1][t % per[0]] for t in range(K + 6))
        assert coded_bits(K, rate) == want == keep_mask(K, rate).sum() == len(_scalar_encode([0] * K, rate))
    rng = np.random.default_rng(1)
    for K in (1, 5, 13):
        u = rng.integers(0, 2, K)
        assert conv_encode(u, rate).tolist() == _scalar_encode(u, rate)
    assert (coded_bits(512, "1/2"), coded_bits(512, "3/4"), coded_bits(1024, "3/4")) == (1036, 691, 1374)


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
@pytest.mark.parametrize("rate", RATES)
def test_noiseless_round_trip(rate, m):
    keys = frame_keys(SEED, np.arange(3))
    for name, K in (("odd_30x7", 40), ("edges_24x6", 37), ("full_rows_40x2", 9)):
        code = CodeConfig(LinkConfig(SIMS[name], m), K, rate)
        info, sent = link_encode_host(code, keys)
        assert info.shape == (3, code.blocks, K) and sent.shape == (3, code.blocks, code.coded_bits)
        assert info.tolist() == (words(keys[:, None], STREAM_CODE_BITS, np.arange(code.blocks * K, dtype=np.uint64)[None]) >> np.uint64(63)) \
            .reshape(info.shape).tolist()
        counts, bits = link_decode_host(code, keys, noiseless_llrs(code, keys))
        assert counts.shape == (3, 2) and (counts == 0).all() and (bits == info).all()
        assert link_decode_host(code, keys, -noiseless_llrs(code, keys))[0][:, 1].tolist() == [code.blocks] * 3     # every bit inverted


def _brute_force(z, K, rate):
    """The inputs of the largest metric among all 2^K; of several, the one smallest when read from the last input to the first."""
    mask = keep_mask(K, rate).reshape(-1)
    zk = z.reshape(-1)[mask]
    best = None
    for u in itertools.product((0, 1), repeat=K):
        c = np.array(_scalar_encode(u, rate))
        metric = int(((1 - 2 * c) * zk).sum())
        key = (-metric, u[::-1])
        if best is None or key < best[0]:
            best = (key, u, metric)
    return best[1], best[2]


@pytest.mark.parametrize("rate", RATES)
def test_host_decoder_against_a_brute_force_over_all_inputs(rate):
    rng = np.random.default_rng(7)
    ties = 0
    for K in (1, 2, 3, 5, 8):
        mask = keep_mask(K, rate)
        for trial in range(6 if K < 8 else 3):
            z = (rng.integers(-2, 3, (K + 6, 2)) * mask).astype(np.int32)          # small integers: many ties
            if trial == 0:
                z[:] = 0                                                         # the tie rule decides everything: all-zero inputs win
            got = viterbi_host(z)
            want, metric = _brute_force(z, K, rate)
            assert got[K:].sum() == 0 and tuple(got[:K].tolist()) == want, (K, trial, got, want)
            c = np.array(_scalar_encode(want, rate))
            others = sum(int(((1 - 2 * np.array(_scalar_encode(u, rate))) * z.reshape(-1)[mask.reshape(-1)]).sum()) == metric
                         for u in itertools.product((0, 1), repeat=K))
            ties += others > 1
            assert int(((1 - 2 * c) * z.reshape(-1)[mask.reshape(-1)]).sum()) == metric
    assert ties >= 5                                                             # the tie rule was exercised


def test_link_decode_host_against_a_bit_by_bit_mapping_and_the_brute_force():
    """The mapping of coded bits to LLRs written with loops: the interleaver, the walk over the grid that skips pilots, the word's
    bit, the scrambler; then the brute force on those inputs."""
    rng = np.random.default_rng(11)
    keys = frame_keys(SEED, np.arange(2))
    for name, m, rate, K in (("small_12x4", 2, "1/2", 8), ("small_12x4", 6, "3/4", 7), ("full_rows_40x2", 4, "2/3", 6)):
        code = CodeConfig(LinkConfig(SIMS[name], m), K, rate)
        sim = code.link.sim
        S, T = sim.ofdm
        llr = (rng.integers(-3, 4, (2, S, T, m)) / 8.0).astype(np.float32)
        counts, bits = link_decode_host(code, keys, llr)
        data = [(s, t) for s in range(S) for t in range(T) if not (s in sim.pilot_scs and t in sim.pilot_symbols)]
        info, _ = link_encode_host(code, keys)
        for f in range(2):
            for b in range(code.blocks):
                c = _scalar_encode(info[f, b].tolist(), rate)
                z = []
                for i in range(code.coded_bits):
                    j = ((b * code.coded_bits + i) * code.stride) % code.used_bits
                    (s, t), k = data[j // m], j % m
                    word = int(words(keys[f:f + 1], STREAM_DATA_BITS, s * T + t)[0]) >> (64 - m)
                    w = (word >> (m - 1 - k)) & 1
                    z.append(int(round((1 - 2 * (w ^ c[i])) * float(llr[f, s, t, k]) * 8.0)))
                full = np.zeros((K + 6) * 2, np.int32)
                full[keep_mask(K, rate).reshape(-1)] = z
                want, _ = _brute_force(full.reshape(K + 6, 2), K, rate)
                assert tuple(bits[f, b].tolist()) == want
        wrong = bits != info
        assert counts.tolist() == np.stack([wrong.sum(axis=(1, 2)), wrong.any(axis=2).sum(axis=1)], axis=1).tolist()


def test_interleaver_is_a_bijection_and_the_default_stride_is_coprime():
    for U in range(10, 3000):
        a = default_stride(U)
        assert math.gcd(a, U) == 1 and max(1, math.floor(0.3819660112501051 * U)) <= a < U
        assert all(math.gcd(v, U) != 1 for v in range(max(1, math.floor(0.3819660112501051 * U)), a))
    for name, m, rate, K, stride in (("odd_30x7", 4, "1/2", 40, None), ("edges_24x6", 8, "3/4", 5, None), ("small_12x4", 2, "2/3", 3, 1),
                                     ("small_12x4", 6, "1/2", 11, 9)):
        code = CodeConfig(LinkConfig(SIMS[name], m), K, rate, stride=stride)
        U, j = code.used_bits, code.positions()
        assert j.shape == (code.blocks, code.coded_bits) and sorted(j.reshape(-1).tolist()) == list(range(U))
        assert U == code.blocks * code.coded_bits <= code.link.bits_per_frame < U + code.coded_bits
        assert ((j.reshape(-1) * code.stride_inverse) % U).tolist() == list(range(U))
        assert (code.stride * code.stride_inverse) % U == 1 and code.info_bits_per_frame == code.blocks * K
        if stride is None:
            assert code.stride == default_stride(U)


def test_quantiser_edges():
    f = np.float32
    big = np.finfo(np.float32).max
    lam = np.array([0.0625, -0.0625, 0.1875, -0.1875, 0.3125, 0.0624, 0.0626, np.inf, -np.inf, np.nan, 15.875, 15.9376, 15.94, -15.9376,
                    1e30, -1e30, big, -0.0, 0.0], dtype=f)
    want = [0, 0, 2, -2, 2, 0, 1, 127, -127, 0, 127, 127, 127, -127, 127, -127, 127, 0, 0]      # ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    got = quantise(lam, 8.0)
    assert got.dtype == np.int32 and got.tolist() == want
    assert quantise(np.array([15.8125, 15.81251], f), 8.0).tolist() == [126, 127]            # 126.5 to even, just beyond it up
    assert quantise(np.array([1.0, 3.0], f), 0.5).tolist() == [0, 2]
    # one float32 product: a double product would round 3 * (1/3 as float32) differently from the float32 one at the tie
    x = np.array([np.nextafter(f(0.5), f(1.0))], f)
    assert quantise(x, 1.0).tolist() == [1] and quantise(np.array([0.5], f), 1.0).tolist() == [0]


@pytest.mark.parametrize("poison", (np.nan, 1e30, -np.inf))
def test_filler_and_pilot_llrs_have_no_influence(poison):
    rng = np.random.default_rng(5)
    keys = frame_keys(SEED, np.arange(2))
    for name, m, rate, K in (("odd_30x7", 4, "3/4", 50), ("edges_24x6", 6, "1/2", 31), ("full_rows_40x2", 2, "2/3", 9)):
        code = CodeConfig(LinkConfig(SIMS[name], m), K, rate)
        S, T = code.link.sim.ofdm
        llr = (rng.integers(-16, 17, (2, S, T, m)) / 8.0).astype(np.float32)
        want = link_decode_host(code, keys, llr)
        used = np.zeros(S * T * m, bool)
        j = code.positions().reshape(-1)
        used[np.flatnonzero(code.link.data_mask)[j // m] * m + j % m] = True
        assert used.sum() == code.used_bits < S * T * m
        assert not used.reshape(S, T, m)[~code.link.data_mask].any()
        bad = llr.copy().reshape(2, -1)
        bad[:, ~used] = poison
        got = link_decode_host(code, keys, bad.reshape(llr.shape))
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
        assert code.link.bits_per_frame > code.used_bits                          # there was filler to poison


def test_code_config_validates():
    link = LinkConfig(SIMS["small_12x4"], 2)                                      # 40 data elements, 80 bits
    code = CodeConfig(link, 8)
    assert (code.rate, code.qgain, code.coded_bits, code.blocks, code.used_bits, code.steps) == ("1/2", 8.0, 28, 2, 56, 14)
    assert CodeConfig().info_bits == 1024 and CodeConfig().blocks == 3 and CodeConfig().rate_code == _abi.AFT_LINK_RATE_1_2
    assert [CodeConfig(link, 8, r).rate_code for r in RATES] == [_abi.AFT_LINK_RATE_1_2, _abi.AFT_LINK_RATE_2_3, _abi.AFT_LINK_RATE_3_4]
    assert MAX_INFO_BITS == _abi.AFT_LINK_CODE_MAX_INFO_BITS == 4090
    for bad in (0, -1, 4091, 8.0, "8", True):
        with pytest.raises(ValueError, match="info_bits"):
            CodeConfig(link, bad)
    for bad in ("1/3", 0.5, None, "5/6"):
        with pytest.raises(ValueError, match="rate"):
            CodeConfig(link, 8, bad)
    with pytest.raises(ValueError, match="fewer than the 82 coded bits"):
        CodeConfig(link, 35)                                                     # n = 82 > 80: B = 0
    assert CodeConfig(link, 34).blocks == 1
    for bad in (0, 56, 57, -3, 2.0, True):
        with pytest.raises(ValueError, match="stride"):
            CodeConfig(link, 8, stride=bad)
    for bad in (2, 7, 14, 28):
        with pytest.raises(ValueError, match="not coprime"):
            CodeConfig(link, 8, stride=bad)
    assert CodeConfig(link, 8, stride=55).stride_inverse == 55
    for bad in (0.0, -8.0, float("inf"), float("nan"), 1e39, 1e-50):
        with pytest.raises(ValueError, match="qgain"):
            CodeConfig(link, 8, qgain=bad)
    with pytest.raises(ValueError, match="LinkConfig"):
        CodeConfig(SIMS["small_12x4"], 8)
    with pytest.raises(ValueError, match="CodeConfig"):
        BlockErrorAccumulator(link, "cpu")
    with pytest.raises(ValueError, match="Expected llr of shape"):
        link_decode_host(code, frame_keys(0, np.arange(2)), np.zeros((2, 12, 4, 4), np.float32))


def test_the_new_stream_and_the_binding():
    assert STREAM_CODE_BITS == chansim.STREAM_CODE_BITS == 8 and chansim.STREAM_DATA_NOISE_ANGLE == 7
    assert "aft_link_decode_f32" in _abi.SIGNATURES and "aft_link_decode_f32" in _abi.EXPORTED_SYMBOLS
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_decode_f32") == names.index("aft_link_soft_f32") + 1
    restype, argtypes = _abi.SIGNATURES["aft_link_decode_f32"]
    assert len(argtypes) == 12 and argtypes[5] is argtypes[6] is __import__("ctypes").c_ulonglong and argtypes[7] is __import__("ctypes").c_float
    assert _abi.AFT_ABI_VERSION == 10


# ---- physical sanity: the default grid, m = 4, rate 1/2, K = 512, 20 dB, seed 3, frames 0 .. 3 ----

_sanity = []


def sanity_inputs():
    """(code, keys, sigma, scale, ideal, {"ideal": .., "ls": ..}) made once: 4 frames, 24 blocks."""
    if not _sanity:
        sim = ChannelSimConfig(snr_db=(20.0,))
        ideal, pilots, meta = simulate_frames_host(sim, SEED, np.arange(4))
        ideal, pilots = ideal.astype(np.complex64), pilots.astype(np.complex64)
        code = CodeConfig(LinkConfig(sim, 4), 512, "1/2")
        _sanity.append((code, frame_keys(SEED, np.arange(4)), noise_sigma(meta[:, 0]), llr_scale(meta[:, 0]), ideal,
                        {"ideal": ideal, "ls": ls_interpolate(sim, pilots)}))
    return _sanity[0]


def test_physical_sanity_perfect_csi_has_no_block_error_and_ls_has_18():
    code, keys, sigma, scale, ideal, est = sanity_inputs()
    assert code.blocks * 4 == 24
    blocks = {}
    for which, e in est.items():
        llr = link_llrs_host(code.link, keys, ideal, e, sigma, scale)[1]
        counts, bits = link_decode_host(code, keys, llr)
        blocks[which] = int(counts[:, 1].sum())
        print(which, "bit errors", int(counts[:, 0].sum()), "block errors", blocks[which], "of 24")
    assert blocks == {"ideal": 0, "ls": 18}


def test_block_error_accumulator_and_get_link_bler_on_the_host():
    from adafortitran_amd import ingest
    from adafortitran_amd.evaluation import get_link_bler
    code, keys, sigma, scale, ideal, est = sanity_inputs()
    meta = (torch.arange(4, dtype=torch.float32).reshape(4, 1), torch.full((4, 1), 20.0))
    perfect, ls = BlockErrorAccumulator(code, "cpu", seed=SEED), BlockErrorAccumulator(code, "cpu", seed=SEED)
    assert perfect.result() == 0.0 and perfect.result_throughput() == 0.0          # an empty sweep
    for lo in (0, 3):                                                            # two batches: three frames and one
        hi = 3 if lo == 0 else 4
        m = tuple(t[lo:hi] for t in meta)
        perfect.update(None, torch.from_numpy(ideal[lo:hi]), m)
        ls.update(torch.from_numpy(est["ls"][lo:hi]), torch.from_numpy(ideal[lo:hi]), m)
    assert perfect.frames == ls.frames == 4 and perfect.errors.tolist() == [0, 0] and ls.errors[1].item() == 18
    assert perfect.result() == 0.0 and ls.result() == 18 / 24
    assert perfect.result_ber() == 0.0 and ls.result_ber() == ls.errors[0].item() / (24 * 512) > 0
    full = 6 * 512 / code.link.data_elements
    assert perfect.result_throughput() == pytest.approx(full) and ls.result_throughput() == pytest.approx(full * 6 / 24)
    # the sweep: perfect channel knowledge over a pack at 20 dB has no block error; the pack's LS estimate through a model does
    sim = code.link.sim
    pack = make_pack(sim, 4, seed=SEED, snr_db=20.0)
    loaders = [("SNR_20", ingest.ResidentLoader(pack, sim.pilot, 4, device="cpu", shuffle=False))]
    assert get_link_bler(None, loaders, code, seed=SEED) == {20: 0.0}

    class Ls(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("anchor", torch.zeros(1))

        def forward(self, pilots):
            return torch.from_numpy(ls_interpolate(sim, pilots.numpy()))

    assert get_link_bler(Ls(), loaders, code, seed=SEED) == {20: 18 / 24}
