from .model_excel import ExCEL_model  # noqa: F401
from .load_attr import attr_aggregate  # noqa: F401
from .init_head import init_decoder_state_dict  # noqa: F401
