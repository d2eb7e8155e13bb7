// zstd_compress_wide.hip -- the wide instantiation of zstd_compress_kernel
// (ZSK_ZSTD_FORMAT_FULL_WIDE) in an object of its own: zstd_compress.hip's
// kernel source compiled again, with the wide kernel's launch and without the
// host entry points (why: see launch_zstd_compress_wide_kernel there).
#define ZSK_ZSTD_COMPRESS_WIDE_OBJECT
#pragma clang diagnostic ignored "-Wunused-function"   // (the subset's block encoder has no caller here)
#include "zstd_compress.hip"
