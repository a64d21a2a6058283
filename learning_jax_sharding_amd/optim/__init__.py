"""``optax`` equivalent."""
from .adam import (  # noqa: F401
    EmptyState, GradientTransformation, ScaleByAdamState, adam, adamw, apply_updates, chain, scale, sgd,
)
from .clip import clip_by_global_norm, global_norm  # noqa: F401
from .schedule import (  # noqa: F401
    constant_schedule, cosine_decay_schedule, linear_schedule, warmup_cosine_decay_schedule,
)
from .losses import softmax_cross_entropy_with_integer_labels  # noqa: F401
