"""Float64 restatement of the moving average of the weights inside the detector's update (``ldit_adamw_ema_groups_multi_f32``,
DESIGN section 36), on top of tests/optim_oracle.py: the decay of a step and one update of a shadow.  Plain Python / numpy."""
import numpy as np

from tests import optim_oracle as oo        # noqa: F401  (the state machine and AdamW the averaged weights come from)


def ema_decay_at(step, decay, warmup=True):
    """The decay of the update that is the ``step``-th TAKEN one (1-based, as ``state["step"]`` reads after ``advance``)."""
    decay = float(decay)
    return min(decay, (1.0 + step) / (10.0 + step)) if warmup else decay


def ema_weight(step, decay, warmup=True):
    """What the kernel multiplies by: 1 - decay in double, rounded to float once."""
    return float(np.float32(1.0 - ema_decay_at(step, decay, warmup)))


def ema(e, p, d):
    """One update of the shadow ``e`` towards the new parameter ``p`` with decay ``d``, in float64."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + (1.0 - float(d)) * (p - e)
