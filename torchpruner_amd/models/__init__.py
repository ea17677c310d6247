"""Model zoo with the ``forward_partial`` protocol (reference experiments/models/)."""
from .partial import PartialForwardMixin, SequentialPartial, run_stages, with_forward_partial
from .vgg import VGG, get_vgg_model_with_name, make_features, prunable_vgg16, vgg_cifar
from .resnet import ResNet, BasicBlock, Bottleneck, resnet18, resnet34, resnet50, resnet101, resnet152
from .mlp import FCNet, FMNISTConvNet, cifar10_fc, mnist_fc
from .mobilenet import InvertedResidual, MobileNetV2, mobilenet_v2
from .mobilenet_v3 import InvertedResidualV3, MobileNetV3, SqueezeExcitation, mobilenet_v3_large, mobilenet_v3_small

__all__ = [
    "InvertedResidual", "MobileNetV2", "mobilenet_v2",
    "InvertedResidualV3", "MobileNetV3", "SqueezeExcitation", "mobilenet_v3_large", "mobilenet_v3_small",
    "PartialForwardMixin", "SequentialPartial", "run_stages", "with_forward_partial",
    "VGG", "get_vgg_model_with_name", "make_features", "prunable_vgg16", "vgg_cifar",
    "ResNet", "BasicBlock", "Bottleneck", "resnet18", "resnet34", "resnet50", "resnet101", "resnet152",
    "FCNet", "FMNISTConvNet", "cifar10_fc", "mnist_fc",
]
