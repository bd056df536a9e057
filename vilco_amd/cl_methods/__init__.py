from .prompt import Prompt  # noqa: F401
from .coda import CodaPrompt  # noqa: F401
