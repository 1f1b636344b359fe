from .BASNet import BASNet, BasicBlock, RefUnet  # noqa: F401
