"""The LDPC-coded link of ``adafortitran_amd.linksim`` on the CPU: the pinned shifts of the default base matrices, their girth, ``H c = 0``
for the encoder, the decoder's two fixed points (a noiseless codeword, all-zero inputs), the vectorised host decoder against a second
decoder written with scalar loops over the rows of the expanded matrix, ``LdpcConfig``'s refusals, the binding's new names,
``LdpcBlockErrorAccumulator`` / ``get_link_bler`` on the host, and the physical sanity figures.

tests/test_linkldpc_gpu.py compares the kernel with ``link_ldpc_host`` on the grids of tests/test_linkcode.py."""
import ctypes

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, chansim
from adafortitran_amd.chansim import ChannelSimConfig, frame_keys, ls_interpolate, make_pack
from adafortitran_amd.linksim import (LDPC_MAX_EDGES, LDPC_RATES, LDPC_Z, BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator,
                                      LdpcConfig, LinkConfig, default_stride, ldpc_base, ldpc_decode_host, ldpc_encode, ldpc_parity_part,
                                      ldpc_syndrome_ok, link_ldpc_encode_host, link_ldpc_host, link_llrs_host, quantise)
from test_linkcode import SEED, SIMS, noiseless_llrs, sanity_inputs

WIDE = LinkConfig(ChannelSimConfig(), 8)                     # 13248 bits per frame: every code up to n = 2048 fits


def expanded(cfg: LdpcConfig) -> np.ndarray:
    """uint8 ``[64 mb, 64 nb]``: the parity-check matrix, written from the sentence that defines a block."""
    base = cfg.base()
    mb, nb = base.shape
    H = np.zeros((LDPC_Z * mb, LDPC_Z * nb), dtype=np.uint8)
    for i in range(mb):
        for j in range(nb):
            if base[i, j] >= 0:
                for r in range(LDPC_Z):
                    H[LDPC_Z * i + r, LDPC_Z * j + (r + base[i, j]) % LDPC_Z] = 1
    return H


def test_the_pinned_shifts():
    assert ldpc_base(3, 4).tolist() == [[44], [18], [30]]
    assert ldpc_base(4, 6).tolist() == [[44, -1], [18, 24], [30, 38], [-1, 8]]
    row0 = ldpc_base(12, 24)[0]
    assert {int(j): int(row0[j]) for j in np.flatnonzero(row0 >= 0)} == {0: 44, 7: 46, 11: 2}
    assert ldpc_base(12, 24).dtype == np.int32 and (ldpc_base(12, 24, 1) != ldpc_base(12, 24)).any()
    assert ldpc_parity_part(4).tolist() == [[1, 0, -1, -1], [-1, 0, 0, -1], [0, -1, 0, 0], [1, -1, -1, 0]]
    assert LDPC_RATES == {"1/2": (12, 24), "2/3": (8, 24), "3/4": (6, 24)}
    for rate, (mb, nb) in LDPC_RATES.items():
        cfg = LdpcConfig(WIDE, rate)
        assert (cfg.base_rows, cfg.base_cols, cfg.coded_bits, cfg.info_bits) == (mb, nb, 1536, 64 * (nb - mb))
        assert cfg.shifts == tuple(map(tuple, ldpc_base(mb, nb).tolist())) and (cfg.base()[:, nb - mb:] == ldpc_parity_part(mb)).all()


def test_the_search_never_runs_out_and_every_column_has_three_entries():
    n = 0
    for mb in range(3, 17):
        for nb in range(mb + 1, 33):
            for seed in (0, 1, 12345):
                table = ldpc_base(mb, nb, seed)
                assert table.shape == (mb, nb - mb) and ((table >= 0).sum(axis=0) == 3).all() and table.min() >= -1 and table.max() < 64
                n += 1
    assert n == 945


@pytest.mark.parametrize("rate", ("1/2", "2/3", "3/4", (3, 4), (16, 32), (3, 32)))
def test_girth_no_two_rows_share_two_columns_and_a_layer_shares_no_variable(rate):
    cfg = LdpcConfig(WIDE, rate)
    H = expanded(cfg).astype(np.int64)
    overlap = H @ H.T
    np.fill_diagonal(overlap, 0)
    assert overlap.max() <= 1
    assert H.sum() == LDPC_Z * cfg.edges and cfg.edges <= LDPC_MAX_EDGES
    for i, (cols, var) in enumerate(cfg.layers()):
        assert len(np.unique(var)) == var.size == LDPC_Z * len(cols)                    # rows of one layer share no variable
        assert (np.diff(cols) > 0).all() and len(cols) >= 2
        for r in range(LDPC_Z):
            assert sorted(var[:, r].tolist()) == np.flatnonzero(H[LDPC_Z * i + r]).tolist()


@pytest.mark.parametrize("rate", ((3, 4), (4, 6), "1/2", "2/3", "3/4", (5, 9), (16, 32), (3, 32), (16, 17)))
def test_the_encoder_satisfies_every_check(rate):
    cfg = LdpcConfig(WIDE, rate)
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2, (4, cfg.info_bits)).astype(np.uint8)
    c = ldpc_encode(cfg, u)
    assert c.shape == (4, cfg.coded_bits) and c.dtype == np.uint8 and (c[:, :cfg.info_bits] == u).all()
    assert not ((expanded(cfg).astype(np.int64) @ c.T.astype(np.int64)) % 2).any()
    assert ldpc_syndrome_ok(cfg, c).all()
    flipped = c.copy()
    flipped[0, 5] ^= 1
    assert ldpc_syndrome_ok(cfg, flipped).tolist() == [False, True, True, True]
    one = np.zeros(cfg.info_bits, np.uint8)
    one[0] = 1
    assert ldpc_encode(cfg, one).sum() > 1 and ldpc_encode(cfg, np.zeros(cfg.info_bits, np.uint8)).sum() == 0


@pytest.mark.parametrize("rate", ((3, 4), "1/2", "3/4", (16, 32)))
def test_a_noiseless_codeword_decodes_in_one_iteration_and_zeros_stop_at_once(rate):
    cfg = LdpcConfig(WIDE, rate)
    u = np.random.default_rng(4).integers(0, 2, (3, cfg.info_bits)).astype(np.uint8)
    c = ldpc_encode(cfg, u).astype(np.int32)
    for amplitude in (1, 32, 127):
        bits, iterations = ldpc_decode_host(cfg, (1 - 2 * c) * amplitude)
        assert (bits == u).all() and iterations.tolist() == [1, 1, 1] and bits.dtype == np.uint8
    bits, iterations = ldpc_decode_host(cfg, np.zeros((3, cfg.coded_bits), np.int32))
    assert bits.sum() == 0 and iterations.tolist() == [1, 1, 1]
    bits, iterations = ldpc_decode_host(cfg, -(1 - 2 * c[0]) * 9)                       # every bit inverted: the complement is rarely a codeword
    assert iterations.shape == () and bits.shape == (cfg.info_bits,)


def scalar_decode(cfg: LdpcConfig, z, state=None):
    """The definition with scalar loops: the rows of the expanded matrix in order 0 .. 64 mb - 1, each on its own.  ``state``: a dict
    that receives the posteriors ``L``, the messages ``R`` and the ``rows`` they belong to as the decoder leaves them."""
    H = expanded(cfg)
    rows = [np.flatnonzero(h).tolist() for h in H]
    # a row's edges in increasing base column: np.flatnonzero is increasing in the variable, so in the block column
    L = [int(v) for v in z]
    R = [[0] * len(row) for row in rows]
    beta, it = cfg.offset, 0
    for it in range(1, cfg.max_iters + 1):
        for c, row in enumerate(rows):
            Q = [L[v] - R[c][e] for e, v in enumerate(row)]
            mags = [abs(q) for q in Q]
            tot = sum(q < 0 for q in Q) & 1
            m1 = min(mags)
            a = mags.index(m1)
            m2 = min(mags[:a] + mags[a + 1:])
            for e, v in enumerate(row):
                mag = min(max((m2 if e == a else m1) - beta, 0), 127)
                R[c][e] = -mag if tot ^ (Q[e] < 0) else mag
                L[v] = min(max(Q[e] + R[c][e], -8191), 8191)
        x = [1 if v < 0 else 0 for v in L]
        if all(sum(x[v] for v in row) % 2 == 0 for row in rows):
            break
    if state is not None:
        state.update(L=L, R=R, rows=rows)
    return np.array(x[:cfg.info_bits], dtype=np.uint8), it


def _decoder_inputs(cfg, rng):
    """Noisy codewords at the cliff, ties (eighths through the quantiser), saturating values and NaN, garbage."""
    u = rng.integers(0, 2, (6, cfg.info_bits)).astype(np.uint8)
    sign = 1.0 - 2.0 * ldpc_encode(cfg, u)
    noisy = quantise((sign + rng.normal(0, 0.7, sign.shape)) * 2.0, 8.0)
    ties = quantise(sign * rng.integers(-1, 4, sign.shape) / 8.0, 8.0)
    special = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 15.875, 0.0625, -0.1875, 0.0], np.float32)
    wild = quantise(np.where(rng.random(sign.shape) < 0.2, special[rng.integers(0, len(special), sign.shape)], sign * 3.0), 8.0)
    return np.concatenate([noisy[:2], ties[2:4], wild[4:5], quantise(rng.normal(0, 4, sign[5:].shape), 8.0)])


@pytest.mark.parametrize("rate,offset,max_iters", (((3, 4), 4, 20), ((4, 6), 0, 6), ((3, 6), 127, 3), ((5, 8), 1, 4)))
def test_the_host_decoder_equals_a_scalar_decoder_over_the_expanded_rows(rate, offset, max_iters):
    cfg = LdpcConfig(WIDE, rate, offset=offset, max_iters=max_iters)
    z = _decoder_inputs(cfg, np.random.default_rng(21 + offset))
    assert z.min() == -127 and z.max() == 127 and (z == 0).any()
    bits, iterations = ldpc_decode_host(cfg, z)
    for r in range(len(z)):
        want_bits, want_it = scalar_decode(cfg, z[r])
        assert iterations[r] == want_it and (bits[r] == want_bits).all(), (rate, r)
    if max_iters >= 6 and offset < 127:
        assert iterations.min() < max_iters and iterations.max() == max_iters           # some converge, garbage hits the cap


def test_the_posterior_is_the_input_plus_its_messages_and_stays_far_from_its_clamp():
    """L_v = z_v + the sum of the messages into v after every layer, so |L| <= 127 (1 + column weight) <= 127 * 17: the clamp at
    8191 of the definition is a bound of the int16 storage that no input reaches.  Checked on the scalar decoder's state."""
    cfg = LdpcConfig(WIDE, (3, 4), max_iters=9, offset=0)
    z = quantise(np.random.default_rng(8).normal(0, 40, cfg.coded_bits), 8.0)
    assert np.abs(z).max() == 127
    bits, it = ldpc_decode_host(cfg, z)
    state = {}
    want_bits, want_it = scalar_decode(cfg, z, state)
    assert (bits == want_bits).all() and it == want_it == 9
    total = z.astype(np.int64).copy()
    for row, messages in zip(state["rows"], state["R"]):
        total[row] += messages
    assert total.tolist() == state["L"] and np.abs(total).max() > 127
    assert 127 * (1 + (cfg.base() >= 0).sum(axis=0).max()) < 8191 and 127 * 17 < 8191


def test_ldpc_config_validates():
    link = LinkConfig(SIMS["odd_30x7"], 2)                                               # 195 data elements, 390 bits
    cfg = LdpcConfig(link, (3, 4))
    assert (cfg.coded_bits, cfg.info_bits, cfg.blocks, cfg.used_bits, cfg.info_bits_per_frame, cfg.edges) == (256, 64, 1, 256, 64, 10)
    assert (cfg.qgain, cfg.offset, cfg.max_iters, cfg.seed, cfg.stride) == (8.0, 4, 20, 0, default_stride(256))
    assert (cfg.stride * cfg.stride_inverse) % 256 == 1 and sorted(cfg.positions().reshape(-1).tolist()) == list(range(256))
    assert cfg.base().tolist() == [[44, 1, 0, -1], [18, 0, 0, 0], [30, 1, -1, 0]]
    assert LdpcConfig().rate == "1/2" and LdpcConfig().blocks == 4 and LdpcConfig().edges == 61
    assert LdpcConfig(link, (3, 4), seed=5).shifts == tuple(map(tuple, ldpc_base(3, 4, 5).tolist()))
    assert LdpcConfig(link, (3, 4), shifts=[[0], [63], [-1]]).edges == 9 and LDPC_MAX_EDGES == _abi.AFT_LINK_LDPC_MAX_EDGES == 160
    assert LDPC_Z == _abi.AFT_LINK_LDPC_Z == 64
    for bad in ("1/3", "5/6", 0.5, None, (3,), (3, 4, 5)):
        with pytest.raises(ValueError, match="rate"):
            LdpcConfig(link, bad)
    for bad in ((2, 4), (17, 32), (3.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="mb"):
            LdpcConfig(link, bad)
    for bad in ((3, 3), (3, 33), (16, 16), (3, "4")):
        with pytest.raises(ValueError, match="nb"):
            LdpcConfig(link, bad)
    for bad in ([[0], [1]], [[0, 1], [1, 2], [2, 3]], [[0.0], [1.0], [2.0]]):
        with pytest.raises(ValueError, match="an integer table"):
            LdpcConfig(link, (3, 4), shifts=bad)
    for bad in ([[64], [0], [0]], [[-2], [0], [0]]):
        with pytest.raises(ValueError, match="every entry is -1"):
            LdpcConfig(link, (3, 4), shifts=bad)
    with pytest.raises(ValueError, match="base column 1 has no entry"):
        LdpcConfig(WIDE, (3, 5), shifts=[[0, -1], [1, -1], [2, -1]])
    with pytest.raises(ValueError, match="at most 160"):
        LdpcConfig(WIDE, (16, 32), shifts=np.zeros((16, 16), np.int32))                 # 256 + 33 entries
    dense = np.full((16, 16), -1, np.int32)
    dense[:8, :] = 5                                                                    # 128 + 33 = 161
    with pytest.raises(ValueError, match="161 entries"):
        LdpcConfig(WIDE, (16, 32), shifts=dense)
    dense[7, 0] = -1
    assert LdpcConfig(WIDE, (16, 32), shifts=dense).edges == 160
    with pytest.raises(ValueError, match="fewer than the 320 coded bits"):
        LdpcConfig(LinkConfig(SIMS["edges_24x6"], 2), (3, 5))                            # 276 bits per frame
    for bad in (0, 256, 257, -3, 2.0, True):
        with pytest.raises(ValueError, match="stride"):
            LdpcConfig(link, (3, 4), stride=bad)
    for bad in (2, 64, 128):
        with pytest.raises(ValueError, match="not coprime"):
            LdpcConfig(link, (3, 4), stride=bad)
    for bad in (0.0, -8.0, float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError, match="qgain"):
            LdpcConfig(link, (3, 4), qgain=bad)
    for bad in (-1, 128, 4.0, True):
        with pytest.raises(ValueError, match="offset"):
            LdpcConfig(link, (3, 4), offset=bad)
    for bad in (0, 256, 2.0, False):
        with pytest.raises(ValueError, match="max_iters"):
            LdpcConfig(link, (3, 4), max_iters=bad)
    with pytest.raises(ValueError, match="LinkConfig"):
        LdpcConfig(SIMS["odd_30x7"], (3, 4))
    with pytest.raises(ValueError, match="LdpcConfig"):
        LdpcBlockErrorAccumulator(CodeConfig(), "cpu")
    with pytest.raises(ValueError, match="CodeConfig"):
        BlockErrorAccumulator(cfg, "cpu")                                               # the convolutional accumulator is untouched
    with pytest.raises(ValueError, match="Expected llr of shape"):
        link_ldpc_host(cfg, frame_keys(0, np.arange(2)), np.zeros((2, 30, 7, 4), np.float32))
    with pytest.raises(ValueError, match="LdpcConfig"):
        link_ldpc_host(CodeConfig(), frame_keys(0, np.arange(2)), np.zeros((2, 120, 14, 4), np.float32))


def test_the_new_stream_and_the_binding():
    assert chansim.STREAM_LDPC_SHIFTS == 9 and chansim.STREAM_CODE_BITS == 8
    assert "aft_link_ldpc_f32" in _abi.SIGNATURES and "aft_link_ldpc_f32" in _abi.EXPORTED_SYMBOLS
    names = list(_abi.SIGNATURES)
    assert names.index("aft_link_ldpc_f32") == names.index("aft_link_decode_f32") + 1 == names.index("aft_link_soft_f32") + 2
    restype, argtypes = _abi.SIGNATURES["aft_link_ldpc_f32"]
    C = ctypes
    assert restype is C.c_int and len(argtypes) == 15
    assert argtypes == [C.POINTER(_abi.AftLink), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong, C.c_ulonglong,
                        C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert _abi.AFT_ABI_VERSION == 10


def test_the_link_round_trip_and_the_position_on_the_link():
    """Noiseless LLRs decode to the hash's bits in one iteration per block; the positions are the convolutional code's rule; filler
    and pilot LLRs have no influence."""
    keys = frame_keys(SEED, np.arange(3))
    for name, m, rate in (("odd_30x7", 2, (3, 4)), ("odd_30x7", 8, (3, 4)), ("edges_24x6", 4, (3, 4)), ("full_rows_40x2", 6, (4, 6))):
        cfg = LdpcConfig(LinkConfig(SIMS[name], m), rate)
        info, sent = link_ldpc_encode_host(cfg, keys)
        assert info.shape == (3, cfg.blocks, cfg.info_bits) and sent.shape == (3, cfg.blocks, cfg.coded_bits)
        want = chansim.words(keys[:, None], chansim.STREAM_CODE_BITS, np.arange(cfg.info_bits_per_frame, dtype=np.uint64)[None]) >> np.uint64(63)
        assert info.reshape(3, -1).tolist() == want.tolist() and ldpc_syndrome_ok(cfg, sent).all()
        llr = noiseless_llrs(cfg, keys)
        counts, bits = link_ldpc_host(cfg, keys, llr)
        assert counts.dtype == np.int64 and counts.tolist() == [[0, 0, cfg.blocks]] * 3 and (bits == info).all()
        S, T = cfg.link.sim.ofdm
        used = np.zeros(S * T * m, bool)
        j = cfg.positions().reshape(-1)
        assert j.tolist() == [(p * cfg.stride) % cfg.used_bits for p in range(cfg.used_bits)]
        used[np.flatnonzero(cfg.link.data_mask)[j // m] * m + j % m] = True
        assert used.sum() == cfg.used_bits < S * T * m
        rng = np.random.default_rng(5)
        noisy = (llr * rng.normal(0.5, 0.6, llr.shape)).astype(np.float32)
        poisoned = noisy.copy().reshape(3, -1)
        poisoned[:, ~used] = np.nan
        got, want = link_ldpc_host(cfg, keys, poisoned.reshape(llr.shape)), link_ldpc_host(cfg, keys, noisy)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and want[0][:, 2].min() >= cfg.blocks
        inverted = link_ldpc_host(cfg, keys, -llr)[0]
        assert (inverted[:, 1] == cfg.blocks).all() and (inverted[:, 0] > 0).all()


# ---- physical sanity: test_linkcode.sanity_inputs()'s frames (default grid, m = 4, 20 dB, seed 3, frames 0 .. 3) at rate 1/2 ----

_llrs = {}
LS_BLOCK_ERRORS, LS_ITERATIONS = 12, 248                     # of 16 blocks and 16 x 20 iterations: recorded from the host definition


def sanity_llrs(which):
    code, keys, sigma, scale, ideal, est = sanity_inputs()
    if which not in _llrs:
        _llrs[which] = link_llrs_host(code.link, keys, ideal, est[which], sigma, scale)[1]
    return _llrs[which]


def test_physical_sanity_perfect_csi_has_no_block_error_and_ls_has_its_recorded_count():
    """16 blocks of n = 1536 at 20 dB: perfect channel knowledge decodes every block; the interpolated LS estimate, whose LLRs are
    over-confident on its error floor, loses the recorded number of them."""
    code, keys, *_ = sanity_inputs()
    cfg = LdpcConfig(code.link, "1/2")
    assert cfg.blocks == 4 and cfg.info_bits == 768
    result = {}
    for which in ("ideal", "ls"):
        counts, bits = link_ldpc_host(cfg, keys, sanity_llrs(which))
        result[which] = counts.sum(axis=0).tolist()
        print(which, "bit errors", result[which][0], "block errors", result[which][1], "of 16, iterations", result[which][2])
    assert result["ideal"][:2] == [0, 0] and 16 <= result["ideal"][2] < 16 * 20
    assert result["ls"][1] == LS_BLOCK_ERRORS and result["ls"][2] == LS_ITERATIONS


def test_ldpc_accumulator_and_get_link_bler_on_the_host():
    from adafortitran_amd import ingest
    from adafortitran_amd.evaluation import get_link_bler
    code, keys, sigma, scale, ideal, est = sanity_inputs()
    cfg = LdpcConfig(code.link, "1/2")
    meta = (torch.arange(4, dtype=torch.float32).reshape(4, 1), torch.full((4, 1), 20.0))
    perfect, ls = LdpcBlockErrorAccumulator(cfg, "cpu", seed=SEED), LdpcBlockErrorAccumulator(cfg, "cpu", seed=SEED)
    assert perfect.result() == 0.0 and perfect.result_throughput() == 0.0 and perfect.result_iterations() == 0.0     # an empty sweep
    assert perfect.errors.shape == (3,) and perfect.errors.dtype == torch.int64
    for lo, hi in ((0, 3), (3, 4)):                                              # two batches: three frames and one
        m = tuple(t[lo:hi] for t in meta)
        perfect.update(None, torch.from_numpy(ideal[lo:hi]), m)
        ls.update(torch.from_numpy(est["ls"][lo:hi]), torch.from_numpy(ideal[lo:hi]), m)
    want = {w: link_ldpc_host(cfg, keys, sanity_llrs(w))[0].sum(axis=0) for w in ("ideal", "ls")}
    assert perfect.frames == ls.frames == 4 and perfect.errors.tolist() == want["ideal"].tolist() and ls.errors.tolist() == want["ls"].tolist()
    assert perfect.result() == 0.0 and ls.result() == LS_BLOCK_ERRORS / 16
    assert perfect.result_ber() == 0.0 and ls.result_ber() == want["ls"][0] / (16 * 768)
    assert perfect.result_iterations() == want["ideal"][2] / 16 and ls.result_iterations() == LS_ITERATIONS / 16
    full = 4 * 768 / cfg.link.data_elements
    assert perfect.result_throughput() == pytest.approx(full)
    assert ls.result_throughput() == pytest.approx(full * (16 - LS_BLOCK_ERRORS) / 16)
    sim = cfg.link.sim
    pack = make_pack(sim, 4, seed=SEED, snr_db=20.0)
    loaders = [("SNR_20", ingest.ResidentLoader(pack, sim.pilot, 4, device="cpu", shuffle=False))]
    assert get_link_bler(None, loaders, cfg, seed=SEED) == {20: 0.0}
    assert get_link_bler(None, loaders, code, seed=SEED) == {20: 0.0}             # a CodeConfig still runs the Viterbi path

    class Ls(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("anchor", torch.zeros(1))

        def forward(self, pilots):
            return torch.from_numpy(ls_interpolate(sim, pilots.numpy()))

    assert get_link_bler(Ls(), loaders, cfg, seed=SEED) == {20: LS_BLOCK_ERRORS / 16}
