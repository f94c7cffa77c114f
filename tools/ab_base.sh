#!/bin/bash
# build the committed (HEAD) library as ab/base.so for A/B against the working tree:  tools/ab_base.sh [NAME]
exec "$(dirname "$0")/ab_rev.sh" HEAD "${1:-base}"
