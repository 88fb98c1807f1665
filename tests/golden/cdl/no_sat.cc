<?xml version="1.0" encoding="UTF-8"?>
<ColorCorrection id="sop_only">
  <SOPNode>
    <Slope>0.5 0.6 0.7</Slope>
    <Offset>0.25 0.2 0.15</Offset>
    <Power>2.0 1.0 0.5</Power>
  </SOPNode>
</ColorCorrection>
