"""libzseek_amd — MI355X-native random-access decode path of libzseek.

The product is the C-ABI shared library ``libzseek_amd/lib/libzseek.so``
(include/zseek.h + include/zseek_hip.h); this package is its Python host
mirror (``libzseek_amd.zseek``) used by tests and bench.py.
"""
from .zseek import (  # noqa: F401
    ZSEEK_LZ4, ZSEEK_ZSTD, FRAME_DESC_DTYPE, COMPRESS_DESC_DTYPE, LibraryNotBuilt, Reader, Writer, ZseekError,
    decode_frames, frame_batch, kernel_times, kernel_timing, lib, lz4_seekable, parse_kernel_name,
    seek_table_of, status_string, lz4_compress_bound, lz4_compress_frames, lz4_compress_layout,
    lz4_compress_scratch_size, gather_segments, frame_checksums, RANGE_DTYPE, SEGMENT_DTYPE,
    synth_buffer, tools, verify_frame_checksums, with_frame_checksums, zstd_decode_frames,
    zstd_seekable, zstd_tool_version, lz4_image_bound, lz4_build_image,
    zstd_compress_bound, zstd_compress_layout, zstd_compress_scratch_size, zstd_compress_frames,
    zstd_image_bound, zstd_build_image, ZSTD_FORMAT_SUBSET, ZSTD_FORMAT_FULL, IMAGE_ZSTD_FULL,
    ZSTD_FORMAT_FULL_WIDE, IMAGE_ZSTD_WIDE,
    zstd_bounds_default, zstd_decode_frames_async, ERR_SCRATCH,
    lz4_pieces_bound, zstd_pieces_bound, lz4_build_image_pieces, zstd_build_image_pieces,
    IMAGE_FAILED, IMAGE_BAD_PIECES,
    lz4_append_bound, zstd_append_bound, lz4_append_image_pieces, zstd_append_image_pieces,
    IMAGE_BAD_IMAGE, IMAGE_NO_ROOM,
)
