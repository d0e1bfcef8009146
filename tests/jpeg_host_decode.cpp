// Stand-alone host build of the JPEG parser and entropy decoder the library runs (syncfusion_amd/csrc/jpeg_parse.h, jpeg_decode.h):
// decodes the files on its command line and prints, per file, "<status> <checksum>" -- status: ok / unsupported / malformed /
// flagged:<SF_JPEG_ST_* code>; checksum: FNV-1a (64 bit, hex) over the int16 coefficients, component after component, of the blocks the
// decoder reached (tests/jpeg_ref.py, coefficient_checksum).  Always exits 0 unless a file cannot be read: test_jpeg_cpu.py builds it
// with -fsanitize=address,undefined, so a sanitizer report is what fails a run.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../syncfusion_amd/csrc/jpeg_parse.h"

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> file;
    uint8_t chunk[4096];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) file.insert(file.end(), chunk, chunk + got);
    fclose(f);
    // an exact-size heap copy: one byte past either end is a sanitizer report
    uint8_t *bytes = static_cast<uint8_t *>(malloc(file.size() ? file.size() : 1));
    for (size_t i = 0; i < file.size(); ++i) bytes[i] = file[i];
    const int64_t n = (int64_t)file.size();
    sf_jpeg_desc d;
    const int st = sf::jpeg_parse_one(bytes, 0, n, &d);
    if (st != SF_JPEG_OK) {
      printf("%s 0\n", st == SF_JPEG_UNSUPPORTED ? "unsupported" : "malformed");
      free(bytes);
      continue;
    }
    std::vector<sf_jpeg_segment> segs((size_t)d.seg_count);
    sf::jpeg_fill_segments(bytes, &d, 0, segs.data());
    std::vector<int16_t> coef((size_t)sf::jpeg_coef_elems(d), 0);
    int flagged = 0;
    for (const sf_jpeg_segment &g : segs) {
      const int e = sf::jpeg_decode_segment_host(bytes, n, d, g, coef.data());
      if (e && !flagged) flagged = e;
    }
    uint64_t h = 0xCBF29CE484222325ull;
    for (int16_t v : coef) {
      h = (h ^ (uint64_t)((uint16_t)v & 0xFF)) * 0x100000001B3ull;
      h = (h ^ (uint64_t)(((uint16_t)v >> 8) & 0xFF)) * 0x100000001B3ull;
    }
    if (flagged) printf("flagged:%d %016llx\n", flagged, (unsigned long long)h);
    else printf("ok %016llx\n", (unsigned long long)h);
    free(bytes);
  }
  return 0;
}
