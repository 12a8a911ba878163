from .seed import set_seed  # noqa: F401
from .io import load_config, load_nifti, save_nifti  # noqa: F401
from .logger import setup_logger  # noqa: F401
