"""``optax`` equivalent."""
from .adam import (  # noqa: F401
    EmptyState, GradientTransformation, ScaleByAdamState, adam, adamw, apply_updates, chain, scale, sgd,
)
from .losses import softmax_cross_entropy_with_integer_labels  # noqa: F401
