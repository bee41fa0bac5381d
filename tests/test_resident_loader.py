"""ingest.ResidentLoader without a GPU: its order against torch's own DistributedSampler + DataLoader, the epoch semantics, the
values against what the reference's MatDataset produced (tests/golden/I_ingest.npz), the errors raised at construction, and the
argument checks of ``aft_frame_gather_f32`` (every call below is refused before anything is launched)."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset, DistributedSampler

from adafortitran_amd import _abi, _lib, ingest
from test_ingest_eval import I, _write_tree

PS = (12, 2)


def make_pack(n, seed=5, S=120, T=14):
    """A synthetic pack: random targets, the sparse grid non-zero at 12 x 2 pilot positions, distinct meta rows."""
    rng = np.random.default_rng(seed)
    ideal = (rng.standard_normal((n, S, T)) + 1j * rng.standard_normal((n, S, T))).astype(np.complex64)
    sparse = np.zeros((n, S, T), np.complex64)
    rows, cols = np.arange(0, S, S // 12)[:12], np.array([3, 10])
    sparse[:, rows[:, None], cols[None, :]] = ideal[:, rows[:, None], cols[None, :]]
    meta = rng.uniform(0, 30, (n, 5)).astype(np.float32)
    meta[:, 0] = np.arange(n)
    ctype = np.array([("TDL-A", "TDL-B", "CDL-C")[i % 3] for i in range(n)])
    return {"h_ideal": ideal, "h_ls_sparse": sparse, "meta": meta, "channel_type": ctype}


class _Frames(Dataset):
    """The map-style dataset torch's sampler and loader run over: sample i of the packed arrays, in the reference's sample format."""

    def __init__(self, packed):
        self.pilots = torch.from_numpy(ingest.extract_pilots_host(packed["h_ls_sparse"], PS))
        self.ideal = torch.from_numpy(packed["h_ideal"])
        self.meta, self.ctype = packed["meta"], packed["channel_type"]

    def __len__(self):
        return len(self.ideal)

    def __getitem__(self, i):
        m = self.meta[i]
        return self.pilots[i], self.ideal[i], (torch.tensor([m[0]]), torch.tensor([m[1]]), torch.tensor([m[2]]), torch.tensor([m[3]]),
                                              torch.tensor([m[4]]), str(self.ctype[i]))


def _same_batch(got, want):
    pg, ig, mg = got
    pw, iw, mw = want
    assert pg.dtype == torch.complex64 and ig.dtype == torch.complex64
    assert torch.equal(pg, pw) and torch.equal(ig, iw)
    assert len(mg) == 6 and all(torch.equal(a, b) and a.dtype == torch.float32 and a.shape == (pg.shape[0], 1)
                                for a, b in zip(mg[:5], mw[:5]))
    assert tuple(mg[5][0]) == tuple(mw[5])            # the reference's collate gives the strings as one sequence of b


CASES = [(n, w, r, sh, dl) for n in (3, 5, 37, 128) for w in (1, 2, 8) for r in range(w) for sh in (True, False) for dl in (False, True)]


@pytest.mark.parametrize("n", (3, 5, 37, 128))
def test_order_is_torchs_distributed_sampler_and_dataloader(n):
    packed = make_pack(n)
    data = _Frames(packed)
    for (_, w, r, sh, dl) in [c for c in CASES if c[0] == n]:
        loader = ingest.ResidentLoader(packed, PS, 8, device="cpu", shuffle=sh, seed=11, drop_last=dl, rank=r, world_size=w)
        sampler = DistributedSampler(data, num_replicas=w, rank=r, shuffle=sh, seed=11, drop_last=dl)
        ref = DataLoader(data, batch_size=8, sampler=sampler, drop_last=dl)
        for epoch in (0, 3):
            sampler.set_epoch(epoch)
            loader.set_epoch(epoch)
            want = list(ref)
            got = list(loader)
            assert len(got) == len(want) == len(loader), (n, w, r, sh, dl, epoch)
            assert loader.epoch == epoch + 1
            for g, x in zip(got, want):
                _same_batch(g, x)


def test_epoch_order_is_the_samplers_index_list():
    for n, w in ((37, 1), (37, 2), (37, 8), (3, 8)):
        for r in range(w):
            for dl in (False, True):
                s = DistributedSampler(range(n), num_replicas=w, rank=r, shuffle=True, seed=4, drop_last=dl)
                s.set_epoch(2)
                assert ingest.epoch_order(n, 2, True, 4, r, w, dl).tolist() == list(s)


def test_every_iter_is_the_next_epoch_and_set_epoch_rewinds():
    packed = make_pack(37)
    loader = ingest.ResidentLoader(packed, PS, 8, device="cpu", seed=2)
    assert loader.residency == "host" and loader.epoch == 0 and len(loader) == 5
    first = [m[0].flatten().tolist() for _, _, m in loader]
    second = [m[0].flatten().tolist() for _, _, m in loader]
    assert loader.epoch == 2 and first != second
    assert sorted(sum(first, [])) == sorted(sum(second, [])) == list(range(37))      # each a permutation of the pack
    loader.set_epoch(0)
    again = list(loader)
    assert [m[0].flatten().tolist() for _, _, m in again] == first
    loader.set_epoch(0)
    for (p, h, m), k in zip(loader, first):                                          # the frames are those the meta rows name
        sel = np.asarray(k, dtype=np.int64)
        assert np.array_equal(h.numpy(), packed["h_ideal"][sel]) and np.array_equal(m[1].numpy()[:, 0], packed["meta"][sel, 1])
    it0 = iter(loader)                                                               # the epoch is taken when iter() is called
    it1 = iter(loader)
    assert loader.epoch == 3
    assert next(it0)[2][0].flatten().tolist() == second[0] and next(it1)[2][0].flatten().tolist() != second[0]
    plain = ingest.ResidentLoader(packed, PS, 8, device="cpu", shuffle=False, drop_last=True)
    assert len(plain) == 4 and [m[0].flatten().tolist() for _, _, m in plain] == [list(range(i, i + 8)) for i in range(0, 32, 8)]


def test_values_are_the_reference_datasets(tmp_path):
    _write_tree(str(tmp_path))
    ingest.pack_mat_folder(tmp_path / "SNR_10", tmp_path / "snr10.npz")
    sel = [i for i, name in enumerate(I["names"]) if str(name).startswith("SNR_10/")]
    for packed in (str(tmp_path / "snr10.npz"), ingest.pack_mat_folder(tmp_path / "SNR_10")):
        loader = ingest.ResidentLoader(packed, PS, batch_size=2, shuffle=False)
        got = list(loader)
        assert len(got) == len(loader) == 2
        assert np.array_equal(np.concatenate([p.numpy() for p, _, _ in got]), I["pilots"][sel])
        assert np.array_equal(np.concatenate([h.numpy() for _, h, _ in got]), I["ideal"][sel])
        assert np.array_equal(np.concatenate([torch.cat(m[:5], dim=1).numpy() for _, _, m in got]), I["meta"][sel])
        assert not hasattr(loader, "p") and loader.h_ideal.shape == (3, 120, 14) and loader.pilots.shape == (3, 12, 2)


def test_errors_come_at_construction():
    packed = make_pack(9)
    for k in (0, 4, 8):
        bad = dict(packed)
        bad["h_ls_sparse"] = packed["h_ls_sparse"].copy()
        bad["h_ls_sparse"][k, 1, 0] = 1.0                      # a 25th non-zero entry in frame k
        with pytest.raises(ValueError, match=rf"Expected 24 pilot values, got 25 \(frame {k}\)"):
            ingest.ResidentLoader(bad, PS, 4)
    with pytest.raises(ValueError, match="rank"):
        ingest.ResidentLoader(packed, PS, 4, rank=2, world_size=2)
    assert ingest.ResidentLoader(packed, PS, 4).residency == "host"


def test_size_error_names_the_three_sizes_without_a_device():
    """The residency is chosen from the sizes before anything touches the device, so the refusal needs none."""
    packed = make_pack(9)
    need = 9 * (120 * 14 + 24) * 8
    with pytest.raises(ValueError, match=rf"{need} bytes.*max_device_bytes = 10.*max_pinned_bytes = 20.*PackedLoader"):
        ingest.ResidentLoader(packed, PS, 4, device="cuda", max_device_bytes=10, max_pinned_bytes=20)


def test_frame_gather_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                             # host memory, never dereferenced: every call is refused
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    E = _abi.AFT_ERR_ARG

    def refused(rc, word):
        assert rc == E
        assert word in lib.aft_last_error().decode(), lib.aft_last_error()

    good = [p, p, p, p, p, p, 4, 10, 15, 24]
    for k in range(6):
        args = list(good)
        args[k] = None
        refused(lib.aft_frame_gather_f32(*args, None), "NULL")
    for k in range(6, 10):
        for v in (0, -1):
            args = list(good)
            args[k] = v
            refused(lib.aft_frame_gather_f32(*args, None), "bad sizes")
    for k in range(5):
        args = list(good)
        args[k] = p + 4
        refused(lib.aft_frame_gather_f32(*args, None), "8-byte")
    args = list(good)
    args[5] = p + 2
    refused(lib.aft_frame_gather_f32(*args, None), "4-byte")
    assert "aft_frame_gather_f32" in _abi.EXPORTED_SYMBOLS and _abi.AFT_ABI_VERSION == 10
