from .features import FeatureAssembler
from .loader import DeviceLoader, ObservedPairs

__all__ = ["FeatureAssembler", "DeviceLoader", "ObservedPairs"]
