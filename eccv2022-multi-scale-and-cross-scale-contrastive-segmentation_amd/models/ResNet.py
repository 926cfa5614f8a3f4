"""Bottleneck ResNet-50 / ResNet-101 backbones for DeepLabv3, with torchvision's parameter names and its
``replace_stride_with_dilation`` rule, written here because torchvision is not a dependency of this package.

The module holds what torchvision's IntermediateLayerGetter keeps of a ResNet cut after ``layer4`` (``conv1``, ``bn1``, ``relu``,
``maxpool``, ``layer1`` .. ``layer4``; no ``avgpool`` / ``fc``) and returns the dictionary that call yields: ``return_layers`` maps
a layer's name to the key of its output (``{"layer4": "C5"}``, optionally ``layer1`` .. ``layer3`` -> ``C2`` .. ``C4``).

Kernels: the 7x7 stem and the max-pool stay on PyTorch; ``use_kernels()`` moves the 1x1 and the undilated 3x3 convolutions to
DirectConv2d and the dilated 3x3 ones to DilatedConv2d (models/ops_dconv.py).  Norms are never deferred here.

The 1x1 convolution of a strided ``downsample`` is a ``SubsampledConv1x1``: nn.Conv2d with the same attributes (its stride
included), parameters and state_dict, whose forward selects the pixels a 1x1 kernel at that stride reads (``x[:, :, ::2, ::2]``)
and convolves them at stride 1, on the 1x1 kernels of this package where they apply.  On the vendor library the strided form gave
results that changed in the last bit from run to run on the MI355X (tests/test_dconv_hip.py compares two identical steps), and
every layer behind it with them."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils import printlog
from .fused_bn import bn_act

LAYERS = {'resnet50': [3, 4, 6, 3], 'resnet101': [3, 4, 23, 3]}
PAPER_NAMES = {'layer1': 'C2', 'layer2': 'C3', 'layer3': 'C4', 'layer4': 'C5'}


class _AtStride1:
    """What the direct convolution's autograd Function reads of its module, for a SubsampledConv1x1 applied to the map it has
    already subsampled: a 1x1 convolution at stride 1 with that module's weights and fragment cache."""
    stride = (1, 1)
    kernel_size = (1, 1)

    def __init__(self, conv):
        self.conv = conv

    def packed_weights(self):
        from .ops_conv import DirectConv2d
        return DirectConv2d.packed_weights(self.conv)


class SubsampledConv1x1(nn.Conv2d):
    """A 1x1 / stride s / pad 0 convolution as pixel selection + 1x1 convolution at stride 1 (same values: the kernel reads no
    other pixel).  ``direct`` (set by ResNet.use_kernels): contiguous fp32 CUDA inputs take the package's 1x1 kernels."""
    direct = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        assert self.kernel_size == (1, 1) and self.padding == (0, 0) and self.dilation == (1, 1) and self.groups == 1

    def forward(self, x):
        from .amax import refuse_pre
        refuse_pre(x, "SubsampledConv1x1")
        sy, sx = self.stride
        xs = x if (sy, sx) == (1, 1) else x[:, :, ::sy, ::sx].contiguous()
        if (self.direct and xs.is_cuda and xs.dtype == torch.float32 and xs.dim() == 4 and self.weight.dtype == torch.float32
                and not torch.is_autocast_enabled()):
            from .ops_conv import _Conv3x3Direct
            return _Conv3x3Direct.apply(xs, self.weight, _AtStride1(self), None, self.bias)
        return F.conv2d(xs, self.weight, self.bias)


class Bottleneck(nn.Module):
    """1x1 -> 3x3 (carries the stride and the dilation, as torchvision's v1.5 block) -> 1x1 (x4), residual, ReLU."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = bn_act(self.bn1, self.conv1(x))
        out = bn_act(self.bn2, self.conv2(out))
        return bn_act(self.bn3, self.conv3(out), residual=identity)


class ResNet(nn.Module):
    def __init__(self, layers, replace_stride_with_dilation=None, return_layers=None, norm_layer=nn.BatchNorm2d, width=64):
        super().__init__()
        dilate = list(replace_stride_with_dilation) if replace_stride_with_dilation is not None else [False, False, False]
        if len(dilate) != 3:
            raise ValueError(f'replace_stride_with_dilation takes three flags (layer2, layer3, layer4), got {dilate}')
        self.return_layers = dict(return_layers) if return_layers is not None else {'layer4': 'C5'}
        assert set(self.return_layers) <= set(PAPER_NAMES) and 'layer4' in self.return_layers, self.return_layers
        self._norm = norm_layer
        self.inplanes, self.dilation = width, 1
        self.conv1 = nn.Conv2d(3, width, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2, dilate=dilate[0])
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2, dilate=dilate[1])
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2, dilate=dilate[2])
        self.out_channels = width * 8 * Bottleneck.expansion
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.modules.batchnorm._BatchNorm):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride=1, dilate=False):
        """A dilated layer trades its stride for dilation: its first block still runs at the previous dilation (it stands where the
        stride was), the remaining blocks at the new one."""
        previous = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            conv = SubsampledConv1x1 if stride != 1 else nn.Conv2d
            downsample = nn.Sequential(conv(self.inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                                       self._norm(planes * Bottleneck.expansion))
        seq = [Bottleneck(self.inplanes, planes, stride, downsample, previous, self._norm)]
        self.inplanes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            seq.append(Bottleneck(self.inplanes, planes, dilation=self.dilation, norm_layer=self._norm))
        return nn.Sequential(*seq)

    def use_kernels(self):
        from .ops import use_direct_conv1x1, use_direct_conv3x3
        from .ops_dconv import use_dilated_conv3x3
        for name in ('layer1', 'layer2', 'layer3', 'layer4'):
            layer = getattr(self, name)
            use_direct_conv1x1(layer)
            use_direct_conv3x3(layer)
            use_dilated_conv3x3(layer)
        for m in self.modules():
            if isinstance(m, SubsampledConv1x1):
                m.direct = True
        return self

    def forward(self, x):
        x = self.maxpool(bn_act(self.bn1, self.conv1(x)))
        out = OrderedDict()
        for name in ('layer1', 'layer2', 'layer3', 'layer4'):
            x = getattr(self, name)(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def _resnet(arch, pretrained, **kwargs):
    model = ResNet(LAYERS[arch], **kwargs)
    if pretrained:
        path = os.environ.get('RESNET_PRETRAINED', f'{arch}_imagenet_pretrained.pth')
        if not os.path.isfile(path):
            raise FileNotFoundError(f'pretrained {arch} weights not found at {path} (nothing is downloaded; '
                                    'set RESNET_PRETRAINED or use pretrained=False)')
        state = torch.load(path, map_location='cpu')
        state = {k: v for k, v in state.items() if not k.startswith('fc.')}      # the classifier this backbone does not have
        found = model.load_state_dict(state, strict=False)
        missing = [k for k in found.missing_keys if not k.endswith('num_batches_tracked')]
        if missing or found.unexpected_keys:
            # (a checkpoint saved under a prefix such as ``module.`` would otherwise load nothing and train from random weights)
            raise RuntimeError(f'{path} is not a torchvision {arch} state_dict: {len(missing)} missing keys (first: {missing[:3]}), '
                               f'{len(found.unexpected_keys)} unexpected (first: {found.unexpected_keys[:3]})')
        printlog(f'loaded pretrained {arch} from {path}')
    return model


def resnet50(pretrained=False, progress=True, **kwargs):
    return _resnet('resnet50', pretrained, **kwargs)


def resnet101(pretrained=False, progress=True, **kwargs):
    return _resnet('resnet101', pretrained, **kwargs)
