"""CPU tests of the optimised-LAM dispatch of tools/infer_lam (--training_free false): ragged batches go to the batched pipeline's
run_batch_ragged, --api_path true keeps the per-image path, and a model without a decoder head is refused."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle


class _TinyRaggedSet:
    """(name, image u8 [h,w,3], label u8 [h,w], cls f32 [20]) with a different size per sample."""
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def max_k(self):
        return 2

    def __getitem__(self, i):
        rs = np.random.RandomState(500 + i)
        h, w = 5 + i % 7, 4 + (3 * i) % 5
        gt = rs.randint(0, 21, (h, w)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.1] = 255
        cls = np.zeros(20, np.float32)
        cls[i % 20] = 1
        return f"s{i:03d}", rs.randint(0, 256, (h, w, 3)).astype(np.uint8), gt, cls

    def batch(self, idx):
        raise _PerImagePath(idx)


class _PerImagePath(Exception):
    pass


class _StubPipe:
    """Stands in for OptimisedLamPipeline: `labels` = a deterministic function of the image bytes."""
    device, smax = "cpu", 2

    def __init__(self):
        self.hist, self.batches = None, []

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        assert images.numel() == 3 * plan.total_label_pix and gts.numel() == plan.total_label_pix and cls.shape[0] == plan.B
        pred = (images.view(-1, 3)[:, 0].to(torch.int64) % 21).numpy()
        self.hist += torch.from_numpy(oracle.evaluate.fast_hist(gts.numpy(), pred, 21))
        self.batches.append(plan.B)
        return torch.from_numpy(pred.astype(np.uint8))


def _args(*extra):
    from excel_amd.tools import infer_lam
    return infer_lam.get_parser().parse_args(["--batch_size", "5", "--num_workers", "0", "--training_free", "false"] + list(extra))


def test_optimised_regime_runs_ragged_batches_through_the_pipeline(monkeypatch):
    from excel_amd.tools import infer_lam
    for k in ("WORLD_SIZE", "RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    n = 12
    pipe = _StubPipe()
    score, total = infer_lam.validate(_args(), dataset=_TinyRaggedSet(n), pipe=pipe)
    assert pipe.batches == [5, 5, 2]
    ds = _TinyRaggedSet(n)
    ref = sum(oracle.evaluate.fast_hist(ds[i][2].flatten(), ds[i][1].reshape(-1, 3)[:, 0].astype(np.int64) % 21, 21) for i in range(n))
    assert np.array_equal(total.numpy(), ref)


def test_api_path_keeps_the_per_image_sequence(monkeypatch):
    from excel_amd.tools import infer_lam
    for k in ("WORLD_SIZE", "RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    pipe = _StubPipe()
    with pytest.raises(_PerImagePath) as e:
        infer_lam.validate(_args("--api_path", "true"), dataset=_TinyRaggedSet(7), pipe=pipe)
    assert list(e.value.args[0]) == [0]                       # one image per step
    assert pipe.batches == []


def test_model_without_decoder_head_is_refused():
    from excel_amd.pipeline import OptimisedLamPipeline
    from excel_amd.tools import infer_lam
    from excel_amd.utils.PAR import PAR
    no_head = SimpleNamespace(_dec=None)
    with pytest.raises(ValueError, match="decoder"):
        OptimisedLamPipeline(no_head, num_classes=21, smax=2)
    args = _args()
    args.ragged_batches = True
    with pytest.raises(ValueError, match="decoder"):
        infer_lam.build_validation(no_head, PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]), _TinyRaggedSet(3), np.arange(3), "cpu", args)
