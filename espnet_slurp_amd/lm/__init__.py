"""Language models for shallow fusion and perplexity (espnet2/lm)."""
from .espnet_model import ESPnetLanguageModel  # noqa: F401
from .transformer_lm import AbsLM, TransformerLM  # noqa: F401
