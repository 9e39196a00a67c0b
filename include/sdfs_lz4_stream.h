/*
 * sdfs_lz4_stream.h — C-ABI of map files at rest: the LZ4Block stream (GUID.map.lz4) written and
 * read on the MI355X.
 *
 * With Main.COMPRESS_METADATA (Volume.java:257) a closed map file is replaced by
 * CompressionUtils.compressFile(GUID.map) (LongByteArrayMap.close, LongByteArrayMap.java:1003-1015),
 * a snapshot taken without indexing is written as dest.lz4 (LongByteArrayMap.copy, :937-938), a
 * .map.lz4 is expanded by CompressionUtils.decompressFile before its first slot is read
 * (:141-154, :172-177, :464-469), and the cloud stores move every map file through the same two
 * functions (BatchAwsS3ChunkStore.java:2000,2278, BatchAzureChunkStore.java:1306,1404,1804,
 * BatchJCloudChunkStore.java:1423,1553).  compressFile (CompressionUtils.java:127-139) is lz4-java
 * 1.3.0's LZ4BlockOutputStream(fos, 1 << 16, lz4Compressor), decompressFile (:141-151) its
 * LZ4BlockInputStream.
 *
 * The stream: the input cut into blocks of block_size bytes (the last shorter, never empty), each
 *     "LZ4Block" | token | compressedLen LE32 | originalLen LE32 | check LE32 | payload
 * with token = method | level, level = max(0, 32 - clz(block_size - 1) - 10), method 0x20 and the
 * LZ4 block of the data when that is shorter than the data, else 0x10 and the data itself;
 * check = XXH32(data, seed 0x9747b28c) & 0x0FFFFFFF.  The stream ends with a header of method 0x10
 * and three zero ints.  The format is restated from lz4-java 1.3.0's sources; the jar is not part
 * of this project, so the bytes are pinned by the restated model (tests/stream_model.py) only.
 *
 * Every entry point takes the LZ4 handle of sdfs_lz4.h (its mode decides the LZ4 block bytes, its
 * scratch and cross-stream ordering serve the block kernels) and a stream; everything is enqueued,
 * nothing waits on the host.  The handle's device is the one the buffers live on.  Errors, threading
 * and sdfs_cdc_last_error() as in sdfs_lz4.h.
 */
#ifndef SDFS_LZ4_STREAM_H
#define SDFS_LZ4_STREAM_H

#include <stdint.h>

#include "sdfs_lz4.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDFS_CDC_LZ4_STREAM_HEADER_BYTES 21u     /* magic, token, three ints */
#define SDFS_CDC_LZ4_STREAM_SEED 0x9747b28cu     /* LZ4BlockOutputStream.DEFAULT_SEED */
#define SDFS_CDC_LZ4_STREAM_BLOCK 65536u         /* CompressionUtils.compressFile's block size */
#define SDFS_CDC_LZ4_STREAM_MIN_BLOCK 64u        /* LZ4BlockOutputStream.MIN_BLOCK_SIZE */
#define SDFS_CDC_LZ4_STREAM_MAX_BLOCK (1u << 25) /* LZ4BlockOutputStream.MAX_BLOCK_SIZE */
#define SDFS_CDC_LZ4_STREAM_RAW 0x10u            /* COMPRESSION_METHOD_RAW */
#define SDFS_CDC_LZ4_STREAM_LZ4 0x20u            /* COMPRESSION_METHOD_LZ4 */

/* A file's status word: 0, or what is wrong with its first bad block (LZ4BlockInputStream.refill
 * throws there).  The walk stops at that block; the file's output is not to be used. */
#define SDFS_CDC_LZ4_STREAM_TRUNCATED 1u /* header or payload past the file's end, or no end mark (EOFException) */
#define SDFS_CDC_LZ4_STREAM_MAGIC 2u     /* the eight magic bytes differ */
#define SDFS_CDC_LZ4_STREAM_HEADER 4u    /* method, level or lengths refused ("Stream is corrupted") */
#define SDFS_CDC_LZ4_STREAM_DECODE 8u    /* an LZ4 payload does not decode to exactly originalLen bytes */
#define SDFS_CDC_LZ4_STREAM_CHECKSUM 16u /* masked XXH32 of the decoded block != the stored int */
#define SDFS_CDC_LZ4_STREAM_ROOM 32u     /* decompress: decoded length above the room given; nothing written */

/* what the header walk writes per file */
typedef struct sdfs_cdc_lz4_stream_file {
    uint32_t status;      /* SDFS_CDC_LZ4_STREAM_* flags */
    uint32_t n_blocks;    /* data blocks located (before the bad one, if any) */
    uint64_t decoded_len; /* sum of their originalLen */
    uint64_t consumed;    /* bytes up to and including the end mark; position of the bad block otherwise */
} sdfs_cdc_lz4_stream_file;

/* one located data block */
typedef struct sdfs_cdc_lz4_stream_block {
    uint64_t payload_off;    /* in d_data */
    uint32_t compressed_len; /* payload bytes */
    uint32_t original_len;   /* decoded bytes */
    uint32_t method;         /* SDFS_CDC_LZ4_STREAM_RAW / _LZ4 */
    uint32_t check;          /* the stored int */
    uint64_t decoded_off;    /* where the block starts in its file's decoded bytes */
} sdfs_cdc_lz4_stream_block;

/* compressionLevel(blockSize) - COMPRESSION_LEVEL_BASE (LZ4BlockOutputStream): the token's low
 * nibble; -1 for a block size outside 64 .. 2^25. */
int sdfs_cdc_lz4_stream_level(uint32_t block_size);

/* Bytes a stream of n input bytes can take: n + 21 * (ceil(n / block_size) + 1) — the raw
 * fall-back caps every payload at its block's length.  0 for a block size outside 64 .. 2^25. */
uint64_t sdfs_cdc_lz4_stream_bound(uint64_t n, uint32_t block_size);

/* Block-table entries a file of file_len bytes can need: a data block occupies at least 22 bytes. */
uint64_t sdfs_cdc_lz4_stream_max_blocks(uint64_t file_len);

/* StreamingXXHash32 (the stream's Checksum, LZ4BlockOutputStream.flushBufferedData) in bulk:
 * d_out[i] = XXH32(d_data[d_off[i] .. + d_len[i]), seed) for i < *d_count (d_count NULL: i < n_max).
 * Extents may start at any byte. */
int sdfs_cdc_xxh32_device(sdfs_cdc_lz4* z, const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                          const uint32_t* d_count, uint64_t n_max, uint32_t seed, uint32_t* d_out, void* stream);

/* CompressionUtils.compressFile (CompressionUtils.java:127-139) for n_files files at once: file f =
 * d_data[file_off[f] .. + file_len[f]) (host arrays) becomes the stream at d_out + out_off[f]
 * (host array; room sdfs_cdc_lz4_stream_bound(file_len[f], block_size)); d_out_len[f] (device)
 * receives its length.  A file of length 0 yields the end mark alone. */
int sdfs_cdc_lz4_stream_compress_device(sdfs_cdc_lz4* z, const uint8_t* d_data, const uint64_t* file_off,
                                        const uint64_t* file_len, uint32_t n_files, uint32_t block_size,
                                        uint8_t* d_out, const uint64_t* out_off, uint64_t* d_out_len, void* stream);

/* LZ4BlockInputStream.refill's header checks (the part of CompressionUtils.decompressFile,
 * CompressionUtils.java:141-151, that decides where the blocks are) for n_files streams: file f =
 * d_data[file_off[f] .. + file_len[f]) (host arrays).  d_files[f] receives the status, and
 * d_blocks[table_base[f] ..] (host array; room sdfs_cdc_lz4_stream_max_blocks(file_len[f])
 * entries) the located blocks.  Every offset is checked against the file's end before it is used;
 * bytes behind the end mark are not read. */
int sdfs_cdc_lz4_stream_scan_device(sdfs_cdc_lz4* z, const uint8_t* d_data, const uint64_t* file_off,
                                    const uint64_t* file_len, uint32_t n_files, sdfs_cdc_lz4_stream_file* d_files,
                                    sdfs_cdc_lz4_stream_block* d_blocks, const uint64_t* table_base, void* stream);

/* The rest of decompressFile: the blocks the scan located are decoded (LZ4) or copied (RAW) to
 * d_out + out_off[f] + decoded_off (host arrays out_off and out_cap: file f's room) and their
 * XXH32 is compared.  DECODE / CHECKSUM of a file's first such block become d_files[f].status (it
 * lies before the block the header walk stopped at, so it is where LZ4BlockInputStream throws);
 * a file whose status is not 0 afterwards is not to be used.  A file that decodes to more than out_cap[f] bytes gets
 * ROOM and is not touched.  max_blocks bounds the blocks of all files together (the table's size,
 * or their exact number when the caller has read the scan's sizes). */
int sdfs_cdc_lz4_stream_decompress_device(sdfs_cdc_lz4* z, const uint8_t* d_data, uint32_t n_files,
                                          sdfs_cdc_lz4_stream_file* d_files, const sdfs_cdc_lz4_stream_block* d_blocks,
                                          const uint64_t* table_base, uint64_t max_blocks, uint8_t* d_out,
                                          const uint64_t* out_off, const uint64_t* out_cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_LZ4_STREAM_H */
