from .features import FeatureAssembler
from .interactions import Interactions
from .leave_one_out import LeaveOneOut
from .loader import DeviceLoader, ObservedPairs
from .sampler import ItemSampler

__all__ = ["FeatureAssembler", "DeviceLoader", "Interactions", "ItemSampler", "LeaveOneOut", "ObservedPairs"]
