"""The paint rule of vector.PixelSquared, restated in numpy: pixel (y, x) shows grid cell (y*g // height, x*g // width); an empty
cell is 0 in every channel, a target marker (+1) 255 in even channels and 128 in odd ones, the agent (-1) 128 and 255."""
import numpy as np


def render(grid, height, width, channels, channels_last):
    """grid: float array [..., g, g] -> uint8 frames [..., height, width, channels] or [..., channels, height, width]."""
    grid = np.asarray(grid)
    g = grid.shape[-1]
    cells = grid[..., (np.arange(height) * g // height)[:, None], (np.arange(width) * g // width)[None, :]]      # [..., height, width]
    even = np.where(cells > 0, 255, np.where(cells < 0, 128, 0)).astype(np.uint8)
    odd = np.where(cells > 0, 128, np.where(cells < 0, 255, 0)).astype(np.uint8)
    planes = [even if c % 2 == 0 else odd for c in range(channels)]
    return np.stack(planes, axis=-1 if channels_last else -3)
