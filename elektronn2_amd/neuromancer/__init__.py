"""``from elektronn2_amd import neuromancer as nm`` -- the node API of
elektronn2/neuromancer (the subset on the 3-D conv/pool/upconv hot path)."""
from .graphutils import TaggedShape, make_func, floatX, as_floatX
from .variables import VariableParam, VariableWeight, ConstantParam, initweights
from .node_basic import (Node, Input, Input_like, split, SplitPart, Concat, Add, model_manager,
                         choose_name)
from .neural import (Conv, UpConv, Pool, Crop, Pad, AutoMerge, UpConvMerge, FragmentsToDense, Perceptron,
                     LRN)
from .loss import (Softmax, MultinoulliNLL, MalisNLL, SquaredLoss, AbsLoss, BinaryNLL,
                   GaussianNLL, BetaNLL, OneHot, EuclideanDistance, RampLoss, AggregateLoss,
                   Classification, Errors)
from .optimiser import Optimiser, SGD, AdaGrad, AdaDelta, Adam
from .model import Model, modelload, params_from_model_file
from .options import set_plan_options, plan_options
