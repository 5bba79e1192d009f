"""What the accumulation and the two-rank tests of DetectorTrainStep share (tests/test_gpu_detector_accum.py, tests/test_gpu_detector_dp.py,
and the worker processes of the latter): the tiny detector of tests/test_gpu_detector_step.py - hidden 128, 3 layers, 2 heads, 224 x 224 -,
two micro-batches of two images each with the generator seed each is run with, and the single-process reference of an update from both:
``g1 + g2`` made by ``losses -> sum * (1024 * 0.5) -> backward`` and a default ``DetectorTrainStep.apply()`` on it.  No test lives here."""
import numpy as np
import torch

from layoutdit_amd import synth
from layoutdit_amd.config import DiTConfig
from layoutdit_amd.modeling import LayoutDetectionModel
from layoutdit_amd.training import DetectorTrainStep
from tests import rpn_train_oracle as to

DEV = "cuda:0"
SCALE = 1024.0
GEN_SEEDS = (2, 5)                                    # the generator seed micro-batch 0 / 1 is run with


def seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def model():
    """The detector of tests/test_gpu_detector_step.py, identically initialised every time."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    m = LayoutDetectionModel(config=cfg)
    m.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    return m.to(DEV).train()


def micro_batches():
    """[(images, targets)] x 2: the fixture pair of tests/test_gpu_detector_step.py and a second pair from other seeds."""
    def image(h, w, seed):
        return torch.from_numpy(synth.synth_images(1, h, w, seed=seed, kind="uniform")[0]).to(DEV)

    def scene(seed, n, size=(224, 224)):
        return {"boxes": torch.from_numpy(np.ascontiguousarray(to.scene(seed, n, size))).to(DEV),
                "labels": torch.from_numpy(np.arange(n, dtype=np.int64) % 5 + 1).to(DEV)}

    first = ([image(120, 200, 21), image(224, 224, 22)],
             [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=DEV), "labels": torch.tensor([1, 3], device=DEV)},
              scene(7, 7)])
    second = ([image(224, 160, 23), image(200, 224, 24)], [scene(9, 4, (224, 160)), scene(10, 6, (200, 224))])
    return [first, second]


def poisoned(batch):
    """The micro-batch with its first image made of infinities: every loss and every gradient of it is non-finite."""
    images, targets = batch
    return [torch.full_like(images[0], float("inf"))] + list(images[1:]), targets


def grads_of(m, batch, gen_seed, mul):
    """name -> gradient of ``mul * sum(losses)``, cloned, the way DetectorTrainStep.step makes them."""
    for p in m.parameters():
        p.grad = None
    losses = m.losses(*batch, generator=seeded(gen_seed))
    (sum(losses.values()) * mul).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def reference_grads(batches):
    """(g1, g2): the two micro-batches' gradients at ``SCALE * 0.5`` on an identically built model, with their generators."""
    donor = model()
    g1 = grads_of(donor, batches[0], GEN_SEEDS[0], SCALE * 0.5)
    g2 = grads_of(donor, batches[1], GEN_SEEDS[1], SCALE * 0.5)
    assert set(g1) == set(g2)
    return g1, g2


def twin_update(batches, g1, g2, **kw):
    """(twin, its step): a twin model whose p.grad was set to ``g1 + g2`` by hand and updated by a default ``DetectorTrainStep.apply()``
    at the same scale - the same kernels on the same inputs as the accumulating step's update."""
    twin = model()
    grads_of(twin, batches[1], GEN_SEEDS[1], SCALE * 0.5)          # p.grad in the form a backward leaves it (the encoder's: views of one block)
    with torch.no_grad():
        for n, p in twin.named_parameters():
            if p.grad is not None:
                p.grad.copy_(g1[n] + g2[n])
    step = DetectorTrainStep(twin, init_scale=SCALE, **kw)
    step.apply()
    return twin, step
