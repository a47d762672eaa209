/* tests/golden/flac_driver.c -- the fixture generator's hands on libFLAC (tests/golden/make_golden_flac.py builds it
 * against a libFLAC compiled into a temporary directory).  Our code over the public FLAC__stream_encoder_* /
 * FLAC__stream_decoder_* API only.
 *
 *   flac_driver decode in.flac out.pcm out.idx
 *       out.pcm: every decoded sample as int32, interleaved, all channels
 *       out.idx: text.  "info <rate> <channels> <bits> <total> <min_bs> <max_bs>", then per frame
 *                "frame <byte offset in the file> <first sample> <blocksize>", then "end <byte offset behind the last frame>"
 *   flac_driver encode in.pcm <channels> <bits> <rate> <level> <blocksize> out.flac
 *       in.pcm: int32 interleaved
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "FLAC/stream_decoder.h"
#include "FLAC/stream_encoder.h"

typedef struct {
  FILE* pcm;
  FILE* idx;
  FLAC__uint64 frame_start;
  int failed;
} Decode;

static FLAC__StreamDecoderWriteStatus on_write(const FLAC__StreamDecoder* d, const FLAC__Frame* frame, const FLAC__int32* const buffer[],
                                               void* ctx) {
  Decode* s = (Decode*)ctx;
  const unsigned n = frame->header.blocksize, ch = frame->header.channels;
  FLAC__uint64 first = frame->header.number.sample_number, end = 0;
  if (frame->header.number_type == FLAC__FRAME_NUMBER_TYPE_FRAME_NUMBER) first = (FLAC__uint64)frame->header.number.frame_number * n;
  for (unsigned i = 0; i < n; ++i)
    for (unsigned c = 0; c < ch; ++c) fwrite(&buffer[c][i], 4, 1, s->pcm);
  if (!FLAC__stream_decoder_get_decode_position(d, &end)) { s->failed = 1; return FLAC__STREAM_DECODER_WRITE_STATUS_ABORT; }
  fprintf(s->idx, "frame %llu %llu %u\n", (unsigned long long)s->frame_start, (unsigned long long)first, n);
  s->frame_start = end;   /* the decoder stands behind this frame: the next one starts here */
  return FLAC__STREAM_DECODER_WRITE_STATUS_CONTINUE;
}

static void on_metadata(const FLAC__StreamDecoder* d, const FLAC__StreamMetadata* m, void* ctx) {
  Decode* s = (Decode*)ctx;
  (void)d;
  if (m->type == FLAC__METADATA_TYPE_STREAMINFO) {
    const FLAC__StreamMetadata_StreamInfo* i = &m->data.stream_info;
    fprintf(s->idx, "info %u %u %u %llu %u %u\n", i->sample_rate, i->channels, i->bits_per_sample, (unsigned long long)i->total_samples,
            i->min_blocksize, i->max_blocksize);
  }
}

static void on_error(const FLAC__StreamDecoder* d, FLAC__StreamDecoderErrorStatus status, void* ctx) {
  (void)d;
  fprintf(stderr, "libFLAC decoder: %s\n", FLAC__StreamDecoderErrorStatusString[status]);
  ((Decode*)ctx)->failed = 1;
}

static int decode(const char* in, const char* pcm, const char* idx) {
  Decode s;
  memset(&s, 0, sizeof s);
  s.pcm = fopen(pcm, "wb");
  s.idx = fopen(idx, "w");
  FLAC__StreamDecoder* d = FLAC__stream_decoder_new();
  if (!s.pcm || !s.idx || !d) return 2;
  if (FLAC__stream_decoder_init_file(d, in, on_write, on_metadata, on_error, &s) != FLAC__STREAM_DECODER_INIT_STATUS_OK) return 3;
  if (!FLAC__stream_decoder_process_until_end_of_metadata(d) || !FLAC__stream_decoder_get_decode_position(d, &s.frame_start)) return 4;
  const int ok = FLAC__stream_decoder_process_until_end_of_stream(d) && !s.failed;
  fprintf(s.idx, "end %llu\n", (unsigned long long)s.frame_start);
  FLAC__stream_decoder_delete(d);
  fclose(s.pcm);
  fclose(s.idx);
  return ok ? 0 : 5;
}

static int encode(const char* in, unsigned channels, unsigned bits, unsigned rate, unsigned level, unsigned blocksize, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  FLAC__int32* pcm = (FLAC__int32*)malloc(bytes > 0 ? (size_t)bytes : 1);
  if (!pcm || fread(pcm, 1, (size_t)bytes, f) != (size_t)bytes) return 2;
  fclose(f);
  const unsigned frames = (unsigned)(bytes / 4 / channels);
  FLAC__StreamEncoder* e = FLAC__stream_encoder_new();
  if (!e) return 2;
  FLAC__stream_encoder_set_channels(e, channels);
  FLAC__stream_encoder_set_bits_per_sample(e, bits);
  FLAC__stream_encoder_set_sample_rate(e, rate);
  FLAC__stream_encoder_set_compression_level(e, level);
  if (blocksize) FLAC__stream_encoder_set_blocksize(e, blocksize);
  FLAC__stream_encoder_set_total_samples_estimate(e, frames);
  if (FLAC__stream_encoder_init_file(e, out, NULL, NULL) != FLAC__STREAM_ENCODER_INIT_STATUS_OK) return 3;
  const int ok = FLAC__stream_encoder_process_interleaved(e, pcm, frames) && FLAC__stream_encoder_finish(e);
  FLAC__stream_encoder_delete(e);
  free(pcm);
  return ok ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc == 5 && strcmp(argv[1], "decode") == 0) return decode(argv[2], argv[3], argv[4]);
  if (argc == 9 && strcmp(argv[1], "encode") == 0)
    return encode(argv[2], (unsigned)atoi(argv[3]), (unsigned)atoi(argv[4]), (unsigned)atoi(argv[5]), (unsigned)atoi(argv[6]),
                  (unsigned)atoi(argv[7]), argv[8]);
  fprintf(stderr, "usage: flac_driver decode in.flac out.pcm out.idx | encode in.pcm channels bits rate level blocksize out.flac\n");
  return 1;
}
