"""Optimizer / learning-rate schedule factory (host mirror of the reference's common/model_utils.py:17-58).

The returned objects are small descriptors; the arithmetic runs in the fused HIP optimizer kernels
(kws_adam_step / kws_rmsprop_step / kws_sgd_step, and kws_optimizer_step when clipping, momentum, centered or amsgrad is on).
MovingAverage / SWA / Lookahead (get_averaged_optimizer) wrap one of them; their averaging slot is updated inside kws_optimizer_step.
The schedules restate the tf.keras ones the reference picks:
CosineDecay(alpha=0.2), ExponentialDecay(decay_rate=0.9), PolynomialDecay(end = lr/100, power 1),
PiecewiseConstantDecay([500, 0.9*S, S] -> [1e-3, lr, lr/10, lr/100])."""
import math
import struct


class LearningRateSchedule(object):
    def __call__(self, step):
        raise NotImplementedError


class CosineDecay(LearningRateSchedule):
    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0):
        self.initial_learning_rate, self.decay_steps, self.alpha = initial_learning_rate, decay_steps, alpha

    def __call__(self, step):
        s = min(step, self.decay_steps)
        cosine = 0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps))
        return self.initial_learning_rate * ((1 - self.alpha) * cosine + self.alpha)


class ExponentialDecay(LearningRateSchedule):
    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self.initial_learning_rate, self.decay_steps, self.decay_rate, self.staircase = \
            initial_learning_rate, decay_steps, decay_rate, staircase

    def __call__(self, step):
        p = step / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate * self.decay_rate ** p


class PolynomialDecay(LearningRateSchedule):
    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0):
        self.initial_learning_rate, self.decay_steps, self.end_learning_rate, self.power = \
            initial_learning_rate, decay_steps, end_learning_rate, power

    def __call__(self, step):
        s = min(step, self.decay_steps)
        return (self.initial_learning_rate - self.end_learning_rate) * (1 - s / self.decay_steps) ** self.power + \
            self.end_learning_rate


class PiecewiseConstantDecay(LearningRateSchedule):
    def __init__(self, boundaries, values):
        if len(boundaries) != len(values) - 1:
            raise ValueError("The length of boundaries should be 1 less than the length of values")
        self.boundaries, self.values = list(boundaries), list(values)

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


def get_lr_scheduler(learning_rate, decay_type, decay_steps):
    if decay_type:
        decay_type = decay_type.lower()

    if decay_type is None:
        lr_scheduler = learning_rate
    elif decay_type == 'cosine':
        lr_scheduler = CosineDecay(initial_learning_rate=learning_rate, decay_steps=decay_steps, alpha=0.2)
    elif decay_type == 'exponential':
        lr_scheduler = ExponentialDecay(initial_learning_rate=learning_rate, decay_steps=decay_steps, decay_rate=0.9)
    elif decay_type == 'polynomial':
        lr_scheduler = PolynomialDecay(initial_learning_rate=learning_rate, decay_steps=decay_steps,
                                       end_learning_rate=learning_rate / 100)
    elif decay_type == 'piecewise_constant':
        boundaries = [500, int(decay_steps * 0.9), decay_steps]
        values = [0.001, learning_rate, learning_rate / 10., learning_rate / 100.]
        lr_scheduler = PiecewiseConstantDecay(boundaries=boundaries, values=values)
    else:
        raise ValueError('Unsupported lr decay type')

    return lr_scheduler


class Optimizer(object):
    """Descriptor of a Keras optimizer; `kind` selects the HIP update kernel.

    clipvalue / clipnorm / global_clipnorm are the tf.keras optimizer_v2 gradient transformations, applied in that order to the
    gradient after the data-parallel exchange (include/kws.h, kws_optimizer_step).  0 or None is "off"."""
    kind = None

    def __init__(self, learning_rate, clipnorm=None, clipvalue=None, global_clipnorm=None):
        clip = {}
        for name, value in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm)):
            if value is not None and not (float(value) >= 0):
                raise ValueError("`%s` must be >= 0, got %r" % (name, value))
            clip[name] = float(value) if value else None
        if clip["clipnorm"] and clip["global_clipnorm"]:
            raise ValueError("Cannot accept both `clipnorm` and `global_clipnorm`, passed `clipnorm` %r, `global_clipnorm` %r"
                             % (clipnorm, global_clipnorm))
        self.clipnorm, self.clipvalue, self.global_clipnorm = clip["clipnorm"], clip["clipvalue"], clip["global_clipnorm"]
        self.learning_rate = learning_rate
        self.iterations = 0

    @property
    def extended(self):
        """True when an option beyond the bare Keras settings is on: the step then runs kws_optimizer_step instead of the plain kernel"""
        return bool(self.clipnorm or self.clipvalue or self.global_clipnorm)

    def current_lr(self):
        """learning rate for the NEXT update (schedules are evaluated at the number of updates done so far)"""
        lr = self.learning_rate
        return float(lr(self.iterations)) if callable(lr) else float(lr)

    @property
    def lr(self):
        return self.current_lr()

    def set_lr(self, value):
        if callable(self.learning_rate):
            raise TypeError("the learning rate is a schedule and cannot be set")
        self.learning_rate = float(value)


def _check_momentum(momentum):
    if not (0 <= float(momentum) <= 1):
        raise ValueError("`momentum` must be between [0, 1], got %r" % (momentum,))
    return float(momentum)


class Adam(Optimizer):
    kind = 'adam'

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None):
        Optimizer.__init__(self, learning_rate, clipnorm, clipvalue, global_clipnorm)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.amsgrad = bool(amsgrad)

    @property
    def extended(self):
        return self.amsgrad or Optimizer.extended.fget(self)


class RMSprop(Optimizer):
    kind = 'rmsprop'

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None):
        Optimizer.__init__(self, learning_rate, clipnorm, clipvalue, global_clipnorm)
        self.rho, self.epsilon = rho, epsilon
        self.momentum, self.centered = _check_momentum(momentum), bool(centered)

    @property
    def extended(self):
        return self.momentum > 0 or self.centered or Optimizer.extended.fget(self)


class SGD(Optimizer):
    kind = 'sgd'

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None, global_clipnorm=None):
        Optimizer.__init__(self, learning_rate, clipnorm, clipvalue, global_clipnorm)
        self.momentum, self.nesterov = _check_momentum(momentum), bool(nesterov)

    @property
    def extended(self):
        # nesterov without momentum is plain SGD, as in Keras
        return self.momentum > 0 or Optimizer.extended.fget(self)


def get_optimizer(optim_type, learning_rate, average_type=None, decay_type='cosine', decay_steps=100000, **kwargs):
    """kwargs: the optimizer's own options (clipnorm, clipvalue, global_clipnorm; amsgrad; momentum, nesterov, centered), passed
    on to its constructor over the reference's defaults"""
    optim_type = optim_type.lower()

    lr_scheduler = get_lr_scheduler(learning_rate, decay_type, decay_steps)

    if optim_type == 'adam':
        optimizer = Adam(learning_rate=lr_scheduler, **dict(dict(amsgrad=False, clipnorm=None, clipvalue=None), **kwargs))
    elif optim_type == 'rmsprop':
        optimizer = RMSprop(learning_rate=lr_scheduler, **dict(dict(rho=0.9, momentum=0.0, centered=False, clipnorm=None,
                                                                    clipvalue=None), **kwargs))
    elif optim_type == 'sgd':
        optimizer = SGD(learning_rate=lr_scheduler, **dict(dict(momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None),
                                                          **kwargs))
    else:
        raise ValueError('Unsupported optimizer type')

    if average_type:
        # the factory itself stays without averaging (the reference's train.py passes average_type=None too); wrap its result with
        # get_averaged_optimizer(average_type, optimizer) below
        raise ValueError('Unsupported average type')

    return optimizer


AVG_NONE, AVG_BLEND, AVG_SYNC = 0, 1, 2          # include/kws.h KWS_AVG_*


def _f32(x):
    """a double rounded to float32, as the kernel receives it"""
    return struct.unpack('f', struct.pack('f', float(x)))[0]


class AveragedOptimizer(Optimizer):
    """Base of the weight-averaging wrappers (tensorflow-addons' MovingAverage, SWA, Lookahead) around one Optimizer.

    The wrapped optimizer keeps the hyperparameters, the clip options, the learning rate and `iterations`; the wrapper only decides,
    per step, what happens to the averaging slot: average_args(k) -> (mode, alpha) for the update after k earlier ones
    (include/kws.h KWS_AVG_*; alpha computed in double, then rounded to float32).  The slot lives on the device beside the parameters
    (DeviceModel.opt_avg, a copy of them when first needed) and is updated inside kws_optimizer_step, so `extended` is always True."""
    swappable = True       # the slot is an average to evaluate / save with (MovingAverage, SWA); Lookahead's is not

    def __init__(self, optimizer):
        if isinstance(optimizer, AveragedOptimizer):
            raise TypeError("cannot wrap %s: it is an averaging wrapper already" % type(optimizer).__name__)
        if not isinstance(optimizer, Optimizer):
            raise TypeError("optimizer must come from common.model_utils.get_optimizer")
        self.__dict__['optimizer'] = optimizer

    def __getattr__(self, name):       # hyperparameters, clip options, ...: the wrapped optimizer's
        if 'optimizer' not in self.__dict__:
            raise AttributeError(name)
        return getattr(self.__dict__['optimizer'], name)

    kind = property(lambda self: self.optimizer.kind)
    extended = property(lambda self: True)
    iterations = property(lambda self: self.optimizer.iterations, lambda self, v: setattr(self.optimizer, 'iterations', v))
    learning_rate = property(lambda self: self.optimizer.learning_rate, lambda self, v: setattr(self.optimizer, 'learning_rate', v))

    def current_lr(self):
        return self.optimizer.current_lr()

    def set_lr(self, value):
        self.optimizer.set_lr(value)

    def average_args(self, k):
        raise NotImplementedError

    def assign_average_vars(self, model):
        """copy the averages into `model`'s trainable weights for good (tfa's method of that name).  BatchNormalization moving
        statistics have no slot and stay.  Before the first update the averages are the weights: nothing to do."""
        if not self.swappable:
            raise TypeError("%s keeps slow weights, not an average to assign" % type(self).__name__)
        model._assign_average()


def _check_unit(name, value):
    if not (0 <= float(value) <= 1):
        raise ValueError("`%s` must be between [0, 1], got %r" % (name, value))
    return float(value)


def _check_int(name, value, least):
    if int(value) != value or int(value) < least:
        raise ValueError("`%s` must be an integer >= %d, got %r" % (name, least, value))
    return int(value)


class MovingAverage(AveragedOptimizer):
    """exponential moving average of the weights: avg -= (avg - p) (1 - average_decay) after every update from `start_step` on; before
    that the average follows the weights"""

    def __init__(self, optimizer, average_decay=0.99, start_step=0):
        AveragedOptimizer.__init__(self, optimizer)
        self.average_decay, self.start_step = _check_unit("average_decay", average_decay), _check_int("start_step", start_step, 0)

    def average_args(self, k):
        return AVG_BLEND, (1.0 if k < self.start_step else _f32(1.0 - self.average_decay))


class SWA(AveragedOptimizer):
    """stochastic weight averaging: the running mean of the weights after updates start_averaging, start_averaging + average_period, ..."""

    def __init__(self, optimizer, start_averaging=0, average_period=10):
        AveragedOptimizer.__init__(self, optimizer)
        self.start_averaging = _check_int("start_averaging", start_averaging, 0)
        self.average_period = _check_int("average_period", average_period, 1)

    def average_args(self, k):
        d = k - self.start_averaging
        if d < 0 or d % self.average_period:
            return AVG_NONE, 0.0
        return AVG_BLEND, _f32(1.0 / (d // self.average_period + 1))


class Lookahead(AveragedOptimizer):
    """every sync_period updates the slow weights move slow_step_size of the way to the fast ones, and the fast ones restart there"""
    swappable = False

    def __init__(self, optimizer, sync_period=6, slow_step_size=0.5):
        AveragedOptimizer.__init__(self, optimizer)
        self.sync_period = _check_int("sync_period", sync_period, 1)
        self.slow_step_size = _check_unit("slow_step_size", slow_step_size)

    def average_args(self, k):
        if (k + 1) % self.sync_period:
            return AVG_NONE, 0.0
        return AVG_SYNC, _f32(self.slow_step_size)


# the reference's constants for its three average types
AVERAGE_TYPES = {'ema': lambda o: MovingAverage(o, average_decay=0.99),
                 'swa': lambda o: SWA(o, start_averaging=0, average_period=10),
                 'lookahead': lambda o: Lookahead(o, sync_period=6, slow_step_size=0.5)}


def get_averaged_optimizer(average_type, optimizer):
    """`optimizer` under the averaging wrapper `average_type` names ('ema' / 'swa' / 'lookahead', any case), with the constants the
    reference's function of the same name uses; None returns the optimizer as it is"""
    if average_type is None:
        return optimizer
    wrap = AVERAGE_TYPES.get(average_type.lower()) if isinstance(average_type, str) else None
    if wrap is None:
        raise ValueError('Unsupported average type')
    return wrap(optimizer)
