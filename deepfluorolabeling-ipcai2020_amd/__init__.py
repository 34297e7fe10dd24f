"""MI355X-native (gfx950) implementation of the U-Net hot path of rg2/DeepFluoroLabeling-IPCAI2020.

Import as ``dfl_amd`` (see dfl_amd.py at the repository root; this directory's name is not a Python identifier).
Module names mirror the reference's flat files (unet, dice, ncc, util, dataset, warm_restarts_lr).
"""
from . import _native
from .unet import UNet
from .dice import DiceLoss2D, DiceAndHeatMapLoss2D
from .ncc import ncc_2d
from .util import center_crop, get_device
from .warm_restarts_lr import WarmRestartLR
from .optim import SGD, Adam, RMSprop
from . import parallel
from .parallel import DataParallel
from .dataset import DeviceAugment
from . import preprocess
from .preprocess import (out_size, map_lands, unmap_lands, preprocess_projs, preprocess_segs, restore_labels,
                         convert_file)
from . import drr
from .drr import hu_to_mu
from . import register
from . import labels
from . import boundary
from .boundary import DiceBoundaryLoss2D, DiceHeatMapBoundaryLoss2D
from . import ce
from .ce import DiceCELoss2D, DiceHeatMapCELoss2D, balanced_class_weights, cross_entropy_term
from . import tools
from . import synth
from .synth import synthesize

__all__ = ['UNet', 'DiceLoss2D', 'DiceAndHeatMapLoss2D', 'ncc_2d', 'center_crop', 'get_device', 'WarmRestartLR', 'SGD',
           'Adam', 'RMSprop', 'DataParallel', 'parallel', 'DeviceAugment', 'preprocess', 'out_size', 'map_lands', 'unmap_lands',
           'preprocess_projs', 'preprocess_segs', 'restore_labels', 'convert_file', 'drr', 'hu_to_mu', 'register', 'labels', 'tools', 'synth',
           'synthesize', 'boundary', 'DiceBoundaryLoss2D', 'DiceHeatMapBoundaryLoss2D', 'ce',
           'DiceCELoss2D', 'DiceHeatMapCELoss2D', 'balanced_class_weights', 'cross_entropy_term']
