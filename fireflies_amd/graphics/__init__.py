from . import rasterization, depth, components  # noqa: F401
from .components import accept_segmentation, connected_components, connected_components_with_stats  # noqa: F401
