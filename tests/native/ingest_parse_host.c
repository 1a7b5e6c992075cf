// Test infrastructure (tests/test_ingest_parse.py): the device ingest's one-token conversion
// (gulon_amd/csrc/ingest_parse.h), compiled for the host.  Tokens on stdin, one per line (a line ends at \n only, so
// a token may hold \r or blanks; an empty line is the empty token); per token one line out: the binary32's bits as
// eight hex digits, or FLAG.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../gulon_amd/csrc/ingest_parse.h"

int main(void) {
  size_t cap = 1 << 16;
  char *line = malloc(cap);
  long got;
  static char outbuf[1 << 20];
  setvbuf(stdout, outbuf, _IOFBF, sizeof outbuf);
  while ((got = (long)getline(&line, &cap, stdin)) >= 0) {
    if (got > 0 && line[got - 1] == '\n') got--;
    uint32_t bits = 0;
    if (got <= 1 << 20 && gulon_parse_f32((const unsigned char *)line, (int)got, &bits)) printf("%08x\n", bits);
    else puts("FLAG");
  }
  free(line);
  return 0;
}
