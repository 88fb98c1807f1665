<?xml version="1.0" encoding="UTF-8"?>
<ColorCorrection id="bad_power">
  <SOPNode>
    <Slope>1 1 1</Slope>
    <Offset>0 0 0</Offset>
    <Power>1 -0.5 1</Power>
  </SOPNode>
</ColorCorrection>
