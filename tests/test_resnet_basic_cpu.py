"""BasicBlock main nets (ResNet-18 / -34) without a GPU: the restatement tests/basic_ref.py against goldens of the real reference
(tools/gen_golden.py --basic, CPU fp32), the parameter containers against the reference's state_dict names and shapes, ImageNet
initialisation from a torchvision-format resnet18 file, the launcher's -d flag, and the share of gradient tensors the whole-network
GPU parity rule would skip for the two cases."""
import pytest
import torch

from tests.basic_ref import basic_case, manifest_basic, skipped_fraction
from tests.golden_cases_basic import CASES_BASIC, MANIFEST_ONLY, arch_key
from tests.oracle_harness import compare_records, load_golden


@pytest.mark.parametrize("name", list(CASES_BASIC))
def test_restatement_matches_reference_golden(name):
    """Same bound as tests/test_oracle_golden.py: compare_records' rtol 1e-4 on logits / statistics, 2e-3 of the norm on probes."""
    compare_records(basic_case(CASES_BASIC[name]), load_golden(name))


@pytest.mark.parametrize("name", list(CASES_BASIC))
def test_state_dict_equals_reference_manifest(name):
    from adamml_amd.resnet import ResNet
    from tests.golden_cases import CH
    c = CASES_BASIC[name]
    man = manifest_basic(arch_key(c))
    model = ResNet(c["depth"], num_frames=c["groups"], num_classes=31, dropout=0.0, input_channels=CH[c["modality"][0]])
    sd = model.state_dict()
    assert list(sd.keys()) == list(man.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(man[k].shape) and v.dtype == man[k].dtype, k
    assert model.fc.in_features == 512


def test_adamml_depth18_state_dict_equals_reference_manifest():
    from adamml_amd import adamml
    c = MANIFEST_ONLY["adamml18:rgb+sound:lstm"]
    man = manifest_basic(arch_key(c))
    model = adamml(groups=c["groups"], modality=c["modality"], input_channels=[3, 1], num_segments=c["S"], rng_policy=False,
                   rng_threshold=0.5, causality_modeling="lstm", num_classes=31, depth=18, without_t_stride=False, dropout=0.0,
                   pooling_method="max", fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    sd = model.state_dict()
    assert list(sd.keys()) == list(man.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(man[k].shape) and v.dtype == man[k].dtype, k


def test_other_depths_still_raise():
    from adamml_amd.resnet import ResNet
    with pytest.raises(ValueError) as e:
        ResNet(20, num_frames=8)
    for d in ("18", "34", "50", "101", "152"):
        assert d in str(e.value)


def _torchvision_like_resnet18(seed=3):
    """Names and shapes of torchvision's resnet18 state_dict (3-channel stem, 1000-way fc), random values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def bn(p, c):
        sd[p + ".weight"], sd[p + ".bias"] = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
        sd[p + ".running_mean"], sd[p + ".running_var"] = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
        sd[p + ".num_batches_tracked"] = torch.tensor(7)
    sd["conv1.weight"] = torch.randn(64, 3, 7, 7, generator=g)
    bn("bn1", 64)
    inp = 64
    for li, planes in enumerate((64, 128, 256, 512)):
        for bi in range(2):
            p = "layer%d.%d" % (li + 1, bi)
            sd[p + ".conv1.weight"] = torch.randn(planes, inp, 3, 3, generator=g)
            bn(p + ".bn1", planes)
            sd[p + ".conv2.weight"] = torch.randn(planes, planes, 3, 3, generator=g)
            bn(p + ".bn2", planes)
            if bi == 0 and li > 0:
                sd[p + ".downsample.0.weight"] = torch.randn(planes, inp, 1, 1, generator=g)
                bn(p + ".downsample.1", planes)
            inp = planes
    sd["fc.weight"], sd["fc.bias"] = torch.randn(1000, 512, generator=g), torch.randn(1000, generator=g)
    return sd


@pytest.mark.parametrize("cin", [3, 10])
def test_imagenet_init_loads_a_torchvision_resnet18_file(tmp_path, cin):
    """models/resnet.py:251-257 on BasicBlock names: fc dropped (the model keeps its own 31-way head), everything else taken by name,
    a non-RGB 7x7 stem = the mean over RGB repeated; the 3x3 layerN.M.conv1.weight entries (64 -> 64 ones included) stay as they are."""
    from adamml_amd.resnet import resnet
    tv = _torchvision_like_resnet18()
    path = tmp_path / "resnet18-0000.pth"
    torch.save(tv, str(path))
    torch.manual_seed(0)
    model = resnet(18, 31, False, 8, 0.5, "max", cin, imagenet_pretrained=str(path))
    sd = model.state_dict()
    assert tuple(sd["fc.weight"].shape) == (31, 512)
    for k, v in tv.items():
        if k.startswith("fc."):
            continue
        if k == "conv1.weight" and cin != 3:
            want = v.mean(dim=1, keepdim=True).expand(64, cin, 7, 7)
        else:
            want = v
        assert k in sd and torch.equal(sd[k], want.to(sd[k].dtype)), k
    assert set(sd) - set(tv) == set()


def test_launcher_accepts_depth_18_and_keeps_its_default():
    from adamml_amd import train
    assert train.arg_parser().parse_args(["-d", "18"]).depth == 18
    assert train.arg_parser().parse_args(["-d", "34"]).depth == 34
    assert train.arg_parser().parse_args([]).depth == 50


@pytest.mark.parametrize("name", list(CASES_BASIC))
def test_parity_rule_skips_at_most_a_quarter_of_the_gradients(name):
    """tests/test_models_gpu.check_against_emulation leaves out gradient tensors whose bf16-storage emulation is itself decorrelated
    from fp32.  The two GPU parity cases were chosen so that this concerns at most a quarter of their tensors (emulation vs fp32
    needs no GPU)."""
    c = CASES_BASIC[name]
    emu = basic_case(c, emulate_bf16=True, modes=["train"], keep_grads=True)
    ref = basic_case(c, emulate_bf16=False, modes=["train"], keep_grads=True)
    skipped, seen = skipped_fraction(emu, ref)
    print("  %s: %d of %d gradient tensors in the skipped regime" % (name, skipped, seen))
    assert seen > 0 and 4 * skipped <= seen, (skipped, seen)
