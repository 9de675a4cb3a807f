"""hilcodec_amd — MI355X-native (gfx950) HILCodec encode -> RVQ -> decode forward path.

Importing the package loads `lib/libhilcodec_amd.so` (hand-written HIP kernels behind a C ABI,
`include/hilcodec_amd.h`) and fails loudly if it is missing: there is no CPU or PyTorch fallback."""
from . import _lib  # noqa: F401  (raises if the HIP library is not built)
from .models.hilcodec.models import HILCodec  # noqa: F401
# the offline converter; the module's other names are imported from it by name (`from hilcodec_amd.resample import design`)
from .resample import Resampler, resample  # noqa: F401
# the room mixer's eager one-call form and its configuration (the graphed form: graph_step.GraphedDecodeHop(mix=MixConfig(...)))
from .mixer import MixConfig  # noqa: F401
from .ops import room_mix as mix_rooms  # noqa: F401
# the selective forwarding hop: its definition (import it by name), its configuration and the hop object
from . import forward  # noqa: F401
from .forward import ForwardConfig  # noqa: F401
from .graph_step import GraphedForwardHop  # noqa: F401
# its downlink control (rate control and NACK answers per listener): the definition (import it by name) and the configuration
from . import downlink  # noqa: F401
from .downlink import DownlinkConfig  # noqa: F401
# SRTP packet protection: the definition (import it by name), its configuration, and the two launches outside a graph, on any rows
# and state (the graphed form: graph_step.GraphedEncodeHop(srtp=SrtpConfig()) / GraphedDecodeHop(srtp=SrtpConfig()))
from . import srtp  # noqa: F401
from .srtp import SrtpConfig  # noqa: F401
from .ops import srtp_protect, srtp_unprotect  # noqa: F401
# SRTP on the forwarding hop (GraphedForwardHop(srtp=SrtpConfig())): the definition (import it by name) and its egress launch outside a
# graph
from . import forward_srtp  # noqa: F401
from .ops import srtp_protect_routes  # noqa: F401

__all__ = ["HILCodec", "Resampler", "resample", "MixConfig", "mix_rooms", "forward", "ForwardConfig", "GraphedForwardHop", "downlink", "DownlinkConfig",
           "srtp", "SrtpConfig", "srtp_protect", "srtp_unprotect", "forward_srtp", "srtp_protect_routes"]
