from .features import FeatureAssembler
from .loader import DeviceLoader

__all__ = ["FeatureAssembler", "DeviceLoader"]
