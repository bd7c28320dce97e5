"""bench.py --dump-outputs on CPU stand-ins of the model and the embedding: whatever the number of
ranks and the embedding width, all files of all ranks together stay within 64 MB, the row sample
fills most of that budget, and every row written is the table row its id names."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Model:
    """the dense tower of the bench's DLRM at embedding width `dim` (26 slots + the bottom MLP)"""

    def __init__(self, dim):
        import bench
        n_ins = 26 + 1
        widths = [bench.DENSE_DIM] + bench.BOTTOM[:-1] + [dim]
        top = [dim + n_ins * (n_ins - 1) // 2 + 1] + bench.TOP
        self._mods = torch.nn.ModuleDict({
            "bottom": torch.nn.Sequential(*[torch.nn.Linear(a, b) for a, b in zip(widths, widths[1:])]),
            "top": torch.nn.Sequential(*[torch.nn.Linear(a, b) for a, b in zip(top, top[1:])])})

    def get_current_loss(self):
        return 0.6931


class _Embedding:
    """row r of the table holds r in every element"""

    def __init__(self, vocab, dim):
        self._t = torch.arange(vocab, dtype=torch.float32)[:, None].expand(vocab, dim)

    def get_vocabulary_size(self):
        return self._t.shape[0]

    def table(self):
        return self._t


@pytest.mark.parametrize("world,dim", [(1, 128), (1, 512), (1, 2048), (8, 128), (64, 512)])
def test_dump_stays_within_64_mb(tmp_path, world, dim):
    import bench
    m, emb = _Model(dim), _Embedding(400_000, dim)
    for rank in range(world):
        bench.dump_outputs(m, emb, str(tmp_path), rank, world)
    files = sorted(os.listdir(tmp_path))
    total = sum(os.path.getsize(tmp_path / f) for f in files)
    assert total <= 64 * 10 ** 6, total
    assert total > 0.95 * 64 * 10 ** 6, total  # the budget goes to the row sample
    assert np.load(tmp_path / "loss.npy").dtype == np.float64
    sfx = [f"_rank{r}" for r in range(world)] if world > 1 else [""]
    for s in sfx:
        ids = np.load(tmp_path / f"embedding_row_ids{s}.npy")
        rows = np.load(tmp_path / f"embedding_rows{s}.npy")
        assert ids.dtype == np.float64 and rows.dtype == np.float32
        assert rows.shape == (ids.size, dim) and ids.size > 0
        assert (rows == ids[:, None]).all()
    for f in files:
        assert np.load(tmp_path / f).dtype in (np.float32, np.float64), f


def test_small_vocabulary_is_dumped_whole(tmp_path):
    import bench
    bench.dump_outputs(_Model(128), _Embedding(1000, 128), str(tmp_path), 0, 1)
    assert (np.load(tmp_path / "embedding_row_ids.npy") == np.arange(1000)).all()
