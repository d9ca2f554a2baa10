"""FusedBNAdd and its place in the U-Net's MobileNetV2 blocks, without a GPU."""

import copy
import re

import torch
import torch.nn.functional as F


def test_fused_bn_add_cpu_is_batch_norm_plus_residual():
    from tensorflowonspark_amd.ops.modules import FusedBNAdd
    torch.manual_seed(0)
    bn = FusedBNAdd(24, eps=1e-3, momentum=0.2)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 2.0)
        bn.bias.uniform_(-1.0, 1.0)
    x, res = torch.randn(3, 24, 5, 7), torch.randn(3, 24, 5, 7)
    for training in (True, False):
        bn.train(training)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        want = F.batch_norm(x, rm, rv, bn.weight, bn.bias, training, 0.2,
                            1e-3) + res
        assert torch.equal(bn(x, res), want)
        assert torch.equal(bn.running_mean, rm)
        assert torch.equal(bn.running_var, rv)
    assert not FusedBNAdd.RELU and FusedBNAdd.ADD
    scripted = torch.jit.script(copy.deepcopy(bn))
    assert torch.equal(scripted(x, res), bn(x, res))


def test_unet_state_dict_keys_and_blocks():
    from tensorflowonspark_amd.models import unet_mobilenet
    from tensorflowonspark_amd.models.segmentation import InvertedResidual
    from tensorflowonspark_amd.ops.modules import FusedBN, FusedBNAdd
    model = unet_mobilenet()
    keys = list(model.state_dict())
    bn = ["weight", "bias", "running_mean", "running_var",
          "num_batches_tracked"]
    # the second block of the second stage: expand, depthwise, project + skip
    want = (["conv.0.0.weight"] + ["conv.0.1." + k for k in bn]
            + ["conv.1.0.weight"] + ["conv.1.1." + k for k in bn]
            + ["conv.2.weight"] + ["conv.3." + k for k in bn])
    prefix = "encoder.stages.1.1."
    assert [k[len(prefix):] for k in keys if k.startswith(prefix)] == want
    blocks = [m for m in model.modules() if isinstance(m, InvertedResidual)]
    assert len(blocks) == 17 and sum(b.use_res for b in blocks) == 10
    for b in blocks:
        assert type(b.conv[-1]) is (FusedBNAdd if b.use_res else FusedBN)
        assert not any(isinstance(m, torch.nn.BatchNorm2d)
                       for m in b.modules())
    # every block's keys follow the pattern above (expand-less: one pair less)
    pat = re.compile(r"encoder\.stages\.\d\.\d\.conv\.(\d\.)?\d\.\w+$")
    assert all(pat.match(k) for k in keys if k.startswith("encoder.stages."))


def test_unet_scripts_and_matches_eager():
    from tensorflowonspark_amd.models import unet_mobilenet
    torch.manual_seed(1)
    model = unet_mobilenet().eval()
    scripted = torch.jit.script(copy.deepcopy(model))
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad():
        assert (model(x) - scripted(x)).abs().max().item() < 1e-5
