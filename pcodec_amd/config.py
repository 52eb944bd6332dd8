"""Config objects mirroring pco_python/src/config.rs (ModeSpec, DeltaSpec, PagingSpec, ChunkConfig)
and progress.rs (Progress)."""
from dataclasses import dataclass, field

from . import _lib as G


@dataclass(frozen=True)
class ModeSpec:  # chunk_config.rs:13-51, pco_python/src/config.rs:4-46
    kind: int = G.MODE_AUTO
    f64: float = 0.0
    u64: int = 0

    @staticmethod
    def auto(): return ModeSpec(G.MODE_AUTO)

    @staticmethod
    def classic(): return ModeSpec(G.MODE_CLASSIC)

    @staticmethod
    def try_float_mult(base): return ModeSpec(G.MODE_TRY_FLOAT_MULT, f64=float(base))

    @staticmethod
    def try_float_quant(k): return ModeSpec(G.MODE_TRY_FLOAT_QUANT, u64=int(k))

    @staticmethod
    def try_int_mult(base): return ModeSpec(G.MODE_TRY_INT_MULT, u64=int(base))

    @staticmethod
    def try_dict(): return ModeSpec(G.MODE_TRY_DICT)


@dataclass(frozen=True)
class DeltaSpec:  # chunk_config.rs:61-109, pco_python/src/config.rs:48-84
    kind: int = G.DELTA_AUTO
    order: int = 0

    @staticmethod
    def auto(): return DeltaSpec(G.DELTA_AUTO)

    @staticmethod
    def no_op(): return DeltaSpec(G.DELTA_NOOP)

    @staticmethod
    def try_consecutive(order): return DeltaSpec(G.DELTA_TRY_CONSECUTIVE, int(order))

    @staticmethod
    def try_lookback(): return DeltaSpec(G.DELTA_TRY_LOOKBACK)

    @staticmethod
    def try_conv1(order): return DeltaSpec(G.DELTA_TRY_CONV1, int(order))


@dataclass(frozen=True)
class PagingSpec:  # chunk_config.rs:112-182, pco_python/src/config.rs:86-106
    max_page_n: int = 1 << 18
    exact: tuple = None

    @staticmethod
    def equal_pages_up_to(n): return PagingSpec(max_page_n=int(n))

    @staticmethod
    def exact_page_sizes(sizes): return PagingSpec(exact=tuple(int(s) for s in sizes))


@dataclass
class ChunkConfig:  # chunk_config.rs:191-235, pco_python/src/config.rs:108-159
    compression_level: int = 8
    mode_spec: ModeSpec = field(default_factory=ModeSpec.auto)
    delta_spec: DeltaSpec = field(default_factory=DeltaSpec.auto)
    paging_spec: PagingSpec = field(default_factory=PagingSpec)
    enable_8_bit: bool = False
    enable_conv1: bool = False   # extension (PCO_GFX_CFG_CONV1): encode DeltaSpec.try_conv1 instead of refusing it
    enable_dict: bool = False    # extension (PCO_GFX_CFG_DICT): encode ModeSpec.try_dict instead of refusing it
    verify: bool = False         # extension (PCO_GFX_CFG_VERIFY): decode every chunk again behind the encode and compare it with its source, bit for bit

    def to_c(self, wrapped=False):
        # (PagingSpec.exact travels beside the struct: pco_chunk_compressor_new_exact / pco_gfx_simple_compress_into_exact, and
        #  PcoGfxWrappedTask::page_sizes through pcodec_amd.paged.compress_chunks)
        return G.make_config(level=self.compression_level, mode=self.mode_spec.kind, mode_f64=self.mode_spec.f64,
                             mode_u64=self.mode_spec.u64, delta=self.delta_spec.kind, delta_order=self.delta_spec.order,
                             max_page_n=self.paging_spec.max_page_n, enable_8_bit=self.enable_8_bit,
                             conv1=self.enable_conv1, dict=self.enable_dict, verify=self.verify)


ChunkSpec = G.ChunkSpec   # extension (include/pco_gfx.h section 3c): one chunk's RESOLVED mode and delta, with FloatMult's inverse -- what paged.resolve_specs returns and specs= takes


def spec_of(mode_spec, delta_spec, dtype):
    """The ChunkSpec an explicit (ModeSpec, DeltaSpec) pair means for number type `dtype` (a numpy / torch dtype, its name or the type byte): what
    pco_gfx_resolve_chunk_specs answers for an explicit config, which needs no device."""
    import ctypes as C
    cfg = ChunkConfig(mode_spec=mode_spec, delta_spec=delta_spec, enable_8_bit=True).to_c()
    task = G.EncodeTask(None, 1, None, 0, G.dtype_byte(dtype), 0)
    out = ChunkSpec()
    G.check(G.lib().pco_gfx_resolve_chunk_specs(1, C.byref(task), C.addressof(cfg), C.byref(out), None))
    return out


@dataclass
class Progress:  # progress.rs:3-12
    n_processed: int = 0
    finished: bool = False
