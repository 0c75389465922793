 5 10
s01          ATGCGTCTTA
s02          ACGC-TCTTA
s03          AAGC-TCCGA
s04          TAGG-TCCGT
s05          TAGG-TCCCT
