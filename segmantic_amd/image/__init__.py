from . import surfaces  # noqa: F401
