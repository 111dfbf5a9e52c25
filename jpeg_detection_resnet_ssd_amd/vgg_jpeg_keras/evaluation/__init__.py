"""classification_part/vgg_jpeg_keras/evaluation: the classifier's evaluator."""
from .evaluators import Evaluator

__all__ = ["Evaluator"]
